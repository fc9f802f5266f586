"""CPU: the host half of the occlusion-consistent paste (vn_gt_paste_visible) — the
restatement tests/visibility_ref.py against closed forms (bins of hand-picked points, a hand-made ray-cast scene), the
`Visibility` dataclass, the sampler's unchanged draw and its offsets, the label dropping of DeviceCollate.concat and the
entry point's status codes (all decided before the first launch)."""
import ctypes

import numpy as np
import pytest

import gtsample_ref as R
import visibility_ref as V


def _pt(*rows):
    return np.array([list(r) + [0.5] for r in rows], dtype=np.float32)


# nu = 8, nv = 4 over v in [-0.5, 0.5): v_scale = 4, every number exact
SMALL = V.Grid(nu=8, nv=4, v_lo=-0.5, v_hi=0.5, margin=0.0, min_visible=1)


def _bin(face, iv, iu, g=SMALL):
    return (face * g.nv + iv) * g.nu + iu


# (point, expected bin or None, expected depth): shared with tests/test_gpu_gt_visibility.py
def edge_points():
    up, down = np.float32(9), np.float32(-9)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    return [
        # the face diagonals |x| == |y|: the x faces take them, u = +-1 (u = 1 lands in the last column)
        ((5.0, 5.0, 0.0), _bin(0, 2, 7), 5.0), ((5.0, -5.0, 0.0), _bin(0, 2, 0), 5.0),
        ((-5.0, 5.0, 0.0), _bin(2, 2, 7), 5.0), ((-5.0, -5.0, 0.0), _bin(2, 2, 0), 5.0),
        # the axes: u = 0 is the first column of the upper half
        ((7.0, 0.0, 0.0), _bin(0, 2, 4), 7.0), ((0.0, 7.0, 0.0), _bin(1, 2, 4), 7.0),
        ((-7.0, 0.0, 0.0), _bin(2, 2, 4), 7.0), ((0.0, -7.0, 0.0), _bin(3, 2, 4), 7.0),
        # just off the diagonal: the y faces
        ((5.0, np.nextafter(np.float32(5), up), 0.0), _bin(1, 2, 7), float(np.nextafter(np.float32(5), up))),
        ((5.0, np.nextafter(np.float32(-5), down), 0.0), _bin(3, 2, 7), float(np.nextafter(np.float32(5), up))),
        # v == v_lo is the first row; its float32 neighbour below has no bin
        ((2.0, 0.0, -1.0), _bin(0, 0, 4), 2.0), ((1.0, 0.0, np.nextafter(np.float32(-0.5), down)), None, 1.0),
        # the float32 neighbour below v_hi is the last row; v_hi itself has no bin
        ((1.0, 0.0, np.nextafter(np.float32(0.5), down)), _bin(0, 3, 4), 1.0), ((1.0, 0.0, 0.5), None, 1.0),
        ((4.0, 1.0, 1.0), _bin(0, 3, 5), 4.0), ((0.5, -4.0, -1.0), _bin(3, 1, 4), 4.0),
        # the origin, a z-dominant point, non-finite coordinates
        ((0.0, 0.0, 0.0), None, 0.0), ((0.0, 0.0, 3.0), None, 0.0), ((0.1, 0.1, 5.0), None, None), ((0.1, -0.05, -5.0), None, None),
        ((inf, 1.0, 0.0), None, None), ((1.0, -inf, 0.0), None, None), ((1.0, 1.0, inf), None, None), ((1.0, 1.0, -inf), None, None),
        ((nan, 1.0, 0.0), None, None), ((1.0, nan, 0.0), None, None), ((1.0, 1.0, nan), None, None),
        # -0.0: |−0| = 0; "px > 0" is false for it, so (−0, 0, z) would be face 2 — but a == 0 gives no bin
        ((-0.0, 3.0, 0.0), _bin(1, 2, 4), 3.0), ((3.0, -0.0, -0.0), _bin(0, 2, 4), 3.0), ((-0.0, -0.0, 1.0), None, 0.0),
        ((-3.0, -0.0, 0.0), _bin(2, 2, 4), 3.0),
    ]


def test_restatement_bins_of_hand_picked_points():
    pts = edge_points()
    has, idx, depth = V.bin_depth(_pt(*[p for p, _, _ in pts]), SMALL)
    for k, (p, want, d) in enumerate(pts):
        assert bool(has[k]) == (want is not None), (p, has[k])
        assert idx[k] == (-1 if want is None else want), (p, idx[k], want)
        if d is not None:
            assert depth[k] == d and np.float32(depth[k]) == depth[k], p
    assert 0 <= idx[has].min() and idx[has].max() < 4 * SMALL.nv * SMALL.nu
    # the default grid: the row of a point is floor((z / a + 0.47) * (64 / 0.57)), evaluated as written
    g = V.Grid()
    has, idx, _ = V.bin_depth(_pt((10.0, 0.0, -1.0), (10.0, 0.0, 1.0), (10.0, 0.0, -4.75)), g)
    row = int(np.floor((np.float64(-0.1) - np.float64(-0.47)) * (np.float64(64) / (np.float64(0.10) - np.float64(-0.47)))))
    assert has.tolist() == [True, False, False] and idx[0] == (0 * 64 + row) * 512 + 256 and 0 <= row < 64


def ray_cast_scene(g):
    """ground (z = -1.7, out to 70 m) plus a wall at x = 20 m (|y| <= 15, z in [-1.7, 1.5]), one return per bin centre
    of faces 0 (+x) and 1 (+y): every bin a car below can fall into holds a scene point"""
    rows = []
    v_scale = g.nv / (g.v_hi - g.v_lo)
    for face in (0, 1):
        for iv in range(g.nv):
            v = g.v_lo + (iv + 0.5) / v_scale
            for iu in range(g.nu):
                u = (iu + 0.5) / (g.nu // 2) - 1.0
                a_ground = -1.7 / v if v < 0 else np.inf
                a_wall = np.inf
                if face == 0 and abs(20.0 * u) <= 15.0 and -1.7 <= 20.0 * v <= 1.5:
                    a_wall = 20.0
                a = min(a_ground, a_wall)
                if a > 70.0:
                    continue
                rows.append((a, u * a, v * a) if face == 0 else (u * a, a, v * a))
    return _pt(*rows)


def car_face(x0, y0, along_y, n=12):
    """the sensor-facing side of a car as n x 8 points: a vertical plane 1.5 m wide, z in [-1.5, -0.3]"""
    s, z = np.meshgrid(np.linspace(-0.75, 0.75, n), np.linspace(-1.5, -0.3, 8))
    s, z = s.ravel(), z.ravel()
    rows = np.stack([x0 + (0 if along_y else 1) * s, y0 + (1 if along_y else 0) * s, z], 1)
    return _pt(*rows.tolist())


def hand_made_scene():
    g = V.Grid()
    scene = ray_cast_scene(g)
    front = car_face(8.0, 0.0, along_y=True)            # in front of the wall, facing the sensor
    behind = car_face(28.0, 0.0, along_y=True)          # behind the wall
    side = car_face(5.0, 11.0, along_y=False)           # off to the side, on the +y face
    few = _pt((10.0, -8.5, -1.0), (10.0, -8.0, -1.0), (10.0, -7.5, -1.0))          # in the open, but three points only
    boxes = np.array([[10.0, 0.0, -1.75, 1.65, 1.6, 4.0, 0.0], [30.0, 0.0, -1.75, 1.65, 1.6, 4.0, 0.0],
                      [5.0, 12.0, -1.75, 1.65, 1.6, 4.0, np.pi / 2], [12.0, -8.0, -1.75, 1.65, 1.6, 4.0, 0.0]])
    objs = [front, behind, side, few]
    return g, scene, boxes, np.concatenate(objs), V.offsets_of(objs)


def test_restatement_on_a_hand_made_ray_cast_scene():
    g, scene, boxes, obj, off = hand_made_scene()
    assert len(scene) > 20000 and len(obj) == 3 * 96 + 3
    for o in range(4):                                   # the faces lie in their boxes
        assert R.inside(obj[off[o]:off[o + 1]], boxes[o]).all()
    r = V.paste_visible(scene, boxes, obj, off, g)
    assert r["visible"].tolist() == [96, 0, 96, 3] and r["accepted"].tolist() == [True, False, True, False]
    assert r["kept"].tolist() == [96, 0, 96, 0]
    # the shadow of the car in front: ground behind it and the wall behind it, and nothing nearer than the car
    gone = ~r["scene_keep"]
    shadow = gone & ~R.masks(scene, boxes[[0, 2]]).any(0)
    assert r["stats"][1] == shadow.sum() > 0
    ahead = shadow & (np.abs(scene[:, 1]) < 3.0) & (scene[:, 0] > 0)
    assert (ahead & (scene[:, 0] == 20.0)).sum() > 0 and (ahead & (scene[:, 2] == np.float32(-1.7)) & (scene[:, 0] < 20.0)).sum() > 0
    assert (scene[ahead, 0] > 8.3).all()
    side = shadow & (scene[:, 1] > np.abs(scene[:, 0]))
    assert side.sum() > 0 and (scene[side, 1] > 11.3).all()
    # scene points inside a rejected car's box stay
    in_rejected = R.inside(scene, boxes[3])
    assert in_rejected.sum() > 0 and r["scene_keep"][in_rejected].all()
    assert r["stats"][0] == R.masks(scene, boxes[[0, 2]]).any(0).sum() > 0
    k = int(r["scene_keep"].sum())
    assert r["count"] == k + 192 and np.array_equal(r["out"][k:k + 96], obj[:96]) and np.array_equal(r["out"][k + 96:k + 192], obj[192:288])
    assert np.isnan(r["out"][r["count"]:]).all() and np.array_equal(r["out"][:k], scene[r["scene_keep"]])
    # margin = inf and min_visible = 0: the plain paste
    plain = V.paste_visible(scene, boxes, obj, off, V.Grid(margin=np.inf, min_visible=0))
    want, count = R.paste(scene, boxes, obj)
    assert plain["count"] == count and np.array_equal(plain["out"], want, equal_nan=True)
    assert plain["stats"].tolist() == [len(scene) + len(obj) - count, 0]
    # a car behind another pasted car is culled by it, keeps its label (acceptance is scene visibility only), and an
    # object never culls its own points
    second = car_face(14.0, 0.0, along_y=True)
    boxes2 = np.array([boxes[0], [16.0, 0.0, -1.75, 1.65, 1.6, 4.0, 0.0]])
    objs = [obj[:96], second]
    open_scene = scene[scene[:, 0] != 20.0]              # without the wall
    r2 = V.paste_visible(open_scene, boxes2, np.concatenate(objs), V.offsets_of(objs), g)
    assert r2["visible"].tolist() == [96, 96] and r2["accepted"].all() and r2["kept"][0] == 96
    # the 96 points of the nearer car leave most bins of its silhouette empty: exactly the points of the farther car
    # that share a bin with one of them go (6 m behind, margin 0.3 m)
    hit = np.isin(V.bin_depth(second, g)[1], V.bin_depth(obj[:96], g)[1])
    assert 0 < hit.sum() < 96 and np.array_equal(r2["obj_keep"][96:], ~hit) and r2["kept"][1] == 96 - hit.sum()


def test_restatement_owner_rule_on_equal_depths():
    """two objects with a bit-equal nearest depth in one bin: the lower index owns it, and at margin = 0 neither culls the
    other (the comparison is strict); a farther point of the other object in that bin goes"""
    g = V.Grid(nu=8, nv=4, v_lo=-0.5, v_hi=0.5, margin=0.0, min_visible=1)
    obj = _pt((4.0, 0.1, 0.1), (4.0, 0.2, 0.2), (4.0, 0.3, 0.3), (4.5, 0.1, 0.1), (4.0, 0.15, 0.15))
    off = np.array([0, 1, 4, 5], dtype=np.int32)          # object 0: row 0; object 1: rows 1..3; object 2: row 4
    boxes = np.array([[100.0 + 10 * i, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0] for i in range(3)])
    assert len(set(V.bin_depth(obj, g)[1].tolist())) == 1
    r = V.paste_visible(np.zeros((0, 4), np.float32), boxes, obj, off, g)
    assert r["visible"].tolist() == [1, 3, 1] and r["obj_keep"].tolist() == [True, True, True, False, True]
    # with the order turned round the farther point belongs to the owner and stays
    off2 = np.array([0, 4, 5], dtype=np.int32)
    r = V.paste_visible(np.zeros((0, 4), np.float32), boxes[:2], obj, off2, g)
    assert r["obj_keep"].all() and r["kept"].tolist() == [4, 1]


# ---------------------------------------------------------------------------------------------------------------------
# the package's host side
# ---------------------------------------------------------------------------------------------------------------------
def test_visibility_validates_its_fields():
    from voxelnet_amd import gtsample as G
    v = G.Visibility()
    assert (v.nu, v.nv, v.v_lo, v.v_hi, v.margin, v.min_visible) == (512, 64, -0.47, 0.10, 0.3, 5)
    assert v.v_scale == float(np.float64(64) / (np.float64(0.10) - np.float64(-0.47)))
    grid = v.grid()
    assert ctypes.sizeof(grid) == 48 and (grid.nu, grid.nv, grid.v_scale, grid.margin, grid.min_visible) == (512, 64, v.v_scale, 0.3, 5)
    assert G.Visibility(margin=np.inf, min_visible=0).margin == np.inf
    assert G.Visibility(nu=2, nv=1).v_scale > 0 and G.Visibility(nu=2048, nv=256).nu == 2048
    for bad in (dict(nu=0), dict(nu=7), dict(nu=2050), dict(nu=8.0), dict(nv=0), dict(nv=257), dict(nv=True), dict(v_lo=0.2),
                dict(v_lo=-np.inf), dict(v_hi=np.nan), dict(v_lo=0.1, v_hi=0.1), dict(margin=-0.1), dict(margin=np.nan),
                dict(min_visible=-1), dict(min_visible=2.5)):
        with pytest.raises(ValueError):
            G.Visibility(**bad)
    with pytest.raises(ValueError):
        G.GTSampler(G.GTDatabase([]), visibility=0.3)
    assert G.GTSampler(G.GTDatabase([])).visibility is None


def _frame(f):
    from voxelnet_amd import synth
    return synth.synth_cloud("Car", 6000, synth.frame_seed(2, f), 2.3, 35), synth.synth_labels("Car", 6, f)


@pytest.fixture(scope="module")
def ref_db():
    return R.database([(f"{f:06d}", *_frame(f)) for f in range(8, 24)])


def _package_db(ref_entries):
    from voxelnet_amd import gtsample as G
    return G.GTDatabase([G.GTEntry(e["cls"], e["tag"], e["box"].copy(), e["points"].copy(), e["line"]) for e in ref_entries])


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_sampler_with_visibility_draws_the_same_and_fills_offsets(ref_db):
    from voxelnet_amd import gtsample as G
    db = _package_db(ref_db)
    plain = G.GTSampler(db, per_class={"Car": 15})
    vis = G.GTSampler(db, per_class={"Car": 15}, visibility=G.Visibility())
    by_line = {e["line"]: e for e in ref_db}
    for f in range(4):
        _, labels = _frame(f)
        np.random.seed(100 + f)
        a = plain.draw(labels, f"{f:06d}")
        after = np.random.get_state()
        np.random.seed(100 + f)
        b = vis.draw(labels, f"{f:06d}")
        assert _same_state(np.random.get_state(), after)
        assert a.lines == b.lines and a.points.tobytes() == b.points.tobytes() and a.table.tobytes() == b.table.tobytes()
        for p in (a, b):
            assert p.offsets.dtype == np.int32 and p.offsets.shape == (len(p.lines) + 1,) and p.offsets[0] == 0
            assert p.offsets[-1] == len(p.points) and len(p.lines) >= 5
            for o, line in enumerate(p.lines):
                assert np.array_equal(p.points[p.offsets[o]:p.offsets[o + 1]], by_line[line]["points"])
    none = G.GTSampler(db, per_class={"Car": 6}, visibility=G.Visibility()).draw(_frame(0)[1], "000000")
    assert none.offsets.tolist() == [0] and none.lines == []
    # earlier constructions keep working
    old = G.GTSampleParams(G.box_table(np.zeros((0, 7))), np.zeros((0, 4), np.float32), np.zeros((0, 7)), [])
    assert old.offsets is None


@pytest.mark.parametrize("augment", [False, True, "compose"])
def test_label_lines_of_rejected_objects_are_dropped(ref_db, augment):
    """DeviceCollate.concat's label step on a fake counts array: the sample's last len(lines) label lines are the pasted
    ones, one line per input line after either augmentation"""
    from voxelnet_amd import augment as A
    from voxelnet_amd import gtsample as G
    from voxelnet_amd.dataset import drop_rejected_lines
    _, labels = _frame(1)
    np.random.seed(4)
    d = G.GTSampler(_package_db(ref_db), per_class={"Car": 15}).draw(labels, "000001")
    enlarged = list(labels) + d.lines
    g = len(d.lines)
    assert g >= 5
    if augment is True:
        np.random.seed(7)                                    # choice 7..9: box perturbation
        while True:
            params = A.draw_augmentation(enlarged)
            if params.mode == "boxes":
                break
        moved = A.augment_labels(enlarged, params)
    elif augment == "compose":
        moved = A.compose_labels(enlarged, A.draw_compose(enlarged, A.ComposeRecipe()))
    else:
        moved = enlarged
    assert len(moved) == len(enlarged)
    visible = np.array([9, 0, 5, 4, 30] + [7] * (g - 5), dtype=np.int32)
    got = drop_rejected_lines(moved, g, visible, 5)
    want = moved[:len(labels)] + [moved[len(labels) + o] for o in range(g) if o not in (1, 3)]
    assert got == want and len(got) == len(enlarged) - 2
    assert drop_rejected_lines(moved, g, visible, 0) == moved
    assert drop_rejected_lines(moved, g, visible, 10 ** 6) == moved[:len(labels)]
    assert drop_rejected_lines(moved, 0, np.zeros(0, np.int32), 5) == moved
    with pytest.raises(ValueError):
        drop_rejected_lines(moved, g, visible[:-1], 5)
    with pytest.raises(ValueError):
        drop_rejected_lines(moved[:2], 3, visible[:3], 5)


def test_no_cpu_path_for_the_visible_paste():
    import torch
    from voxelnet_amd import _lib
    from voxelnet_amd import gtsample as G
    params = G.GTSampleParams(G.box_table(np.zeros((0, 7))), np.zeros((0, 4), np.float32), np.zeros((0, 7)), [], np.zeros(1, np.int32))
    with pytest.raises(_lib.VoxelnetHipError):
        G.gt_paste_visible_device(torch.zeros((8, 4)), params, G.Visibility())
    with pytest.raises(_lib.VoxelnetHipError):
        G.enqueue_gt_paste_visible(torch.zeros((8, 4)), params, G.Visibility())
    assert ctypes.sizeof(_lib.VnVisGrid) == 48
    assert [f for f, _ in _lib.VnVisGrid._fields_] == ["nu", "nv", "v_lo", "v_hi", "v_scale", "margin", "min_visible", "reserved"]


def test_entry_point_checks_its_arguments_on_the_host():
    """every status below is decided before the first launch: no pointer is dereferenced but the grid and the offsets"""
    from voxelnet_amd import _lib
    from voxelnet_amd import gtsample as G
    lib = _lib.load()
    good = G.Visibility().grid()
    gp = ctypes.byref(good)
    wsb = lib.vn_gt_paste_visible_workspace_bytes
    assert wsb(-1, 0, gp) == 0 and wsb(0, -1, gp) == 0 and wsb(1 << 30, 1 << 30, gp) == 0 and wsb(10, 10, None) == 0
    ws = wsb(1000, 10, gp)
    assert ws >= 4 * 64 * 512 * 12 + 1010 + 4 * (4 + 1) and wsb(0, 0, gp) > 0
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    off = (ctypes.c_int32 * 3)(0, 4, 10)
    off0 = (ctypes.c_int32 * 1)(0)
    E, U, W = -1, -2, -3
    pv = lib.vn_gt_paste_visible

    def call(points=0x1000, n=1000, boxes=0x20000, n_boxes=2, obj=0x10000, m=10, offsets=off, grid=gp, out=0x100000, cap=1010,
             count=a, visible=a + 16, kept=a + 32, stats=a + 48, workspace=0x200000, wbytes=ws):
        return pv(points, n, boxes, n_boxes, obj, m, ctypes.cast(offsets, ctypes.c_void_p) if offsets is not None else None, grid, out,
                  cap, count, visible, kept, stats, workspace, wbytes, None)
    assert call(cap=1009) == E                                              # cap < n + m
    assert call(n=-1) == E and call(m=-1) == E and call(n_boxes=129) == E and call(n_boxes=-1) == E
    assert call(boxes=None) == E and call(points=None) == E and call(obj=None) == E and call(out=None) == E
    assert call(count=None) == E and call(stats=None) == E and call(workspace=None) == E and call(offsets=None) == E
    assert call(visible=None) == E and call(kept=None) == E
    assert call(grid=None) == E
    for field, value in (("nu", 0), ("nu", 7), ("nu", 2050), ("nv", 0), ("nv", 257), ("v_lo", 0.2), ("v_hi", float("nan")),
                         ("v_lo", float("-inf")), ("v_scale", 0.0), ("v_scale", float("inf")), ("margin", -1.0),
                         ("margin", float("nan")), ("min_visible", -1)):
        bad = G.Visibility().grid()
        setattr(bad, field, value)
        assert call(grid=ctypes.byref(bad)) == E, (field, value)
    inf = G.Visibility(margin=float("inf"), min_visible=0).grid()
    assert call(grid=ctypes.byref(inf), points=0x1004) == U                 # +inf is a good margin: the next check speaks
    for bad_off in ((1, 4, 10), (0, 4, 9), (0, 4, 11), (0, 11, 10), (0, -1, 10)):
        assert call(offsets=(ctypes.c_int32 * 3)(*bad_off)) == E, bad_off
    assert call(n_boxes=0, boxes=None, offsets=off0) == E                   # offsets[0] must be m
    assert call(out=0x2000) == E                                            # out overlaps the scene
    assert call(out=0x10010) == E                                           # out overlaps the objects
    assert call(wbytes=ws - 1) == W
    assert call(points=0x1004) == U and call(obj=0x10004) == U and call(out=0x100004) == U and call(boxes=0x20008) == U
    assert call(workspace=0x200008) == U and call(count=a + 2) == U and call(visible=a + 18) == U and call(stats=a + 49) == U
    # (no well-formed call here: it would launch)
