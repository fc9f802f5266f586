"""CPU: the host half of the ground-truth database sampling (voxelnet_amd/gtsample.py) — the restatement
tests/gtsample_ref.py against closed forms, the draw (np.random consumption, tags, min_points, collisions, the 128 cap,
class order) against the restatement, the appended label lines, and the database's save / load round trip.  The
databases here are made by the restatement: the points have no CPU path in the package."""
import numpy as np
import pytest

import gtsample_ref as R


def _pt(*rows):
    return np.array([list(r) + [0.5] for r in rows], dtype=np.float32)


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


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against closed forms
# ---------------------------------------------------------------------------------------------------------------------
def test_restatement_axis_aligned_box():
    box = [10.0, 2.0, -1.0, 1.5, 2.0, 4.0, 0.0]          # l = 4 along x, w = 2 along y, z in [-1, 0.5]
    rng = np.random.default_rng(0)
    cloud = np.concatenate([rng.uniform([6, -1, -2], [14, 5, 1.5], (4000, 3)), np.full((4000, 1), 0.5)], 1).astype(np.float32)
    want = ((np.abs(cloud[:, 0].astype(np.float64) - 10.0) <= 2.0) & (np.abs(cloud[:, 1].astype(np.float64) - 2.0) <= 1.0)
            & (cloud[:, 2] >= -1.0) & (cloud[:, 2] <= 0.5))
    got = R.inside(cloud, box)
    assert 200 < want.sum() < 3000 and np.array_equal(got, want)


def test_restatement_quarter_turn_swaps_l_and_w():
    long_x = [0.0, 0.0, 0.0, 1.0, 2.0, 4.0, 0.0]
    turned = [0.0, 0.0, 0.0, 1.0, 2.0, 4.0, np.pi / 2]    # l now runs along y
    cloud = _pt((1.5, 0.0, 0.5), (0.0, 1.5, 0.5), (0.9, 1.9, 0.5), (1.9, 0.9, 0.5), (1.1, 1.1, 0.5))
    assert R.inside(cloud, long_x).tolist() == [True, False, False, True, False]
    assert R.inside(cloud, turned).tolist() == [False, True, True, False, False]


def test_restatement_faces_edges_corners_are_inside():
    box = [8.0, -4.0, -1.0, 2.0, 2.0, 4.0, 0.0]           # x in [6, 10], y in [-5, -3], z in [-1, 1]: all exact in float32
    face, edge, corner = (10.0, -4.0, 0.0), (10.0, -3.0, 0.0), (10.0, -3.0, 1.0)
    cloud = _pt(face, edge, corner, (6.0, -5.0, -1.0), (8.0, -4.0, 1.0), (8.0, -4.0, -1.0))
    assert R.inside(cloud, box).all()
    up = np.float32(99)
    out = _pt((np.nextafter(np.float32(10), up), -4.0, 0.0), (8.0, np.nextafter(np.float32(-3), up), 0.0),
              (8.0, -4.0, np.nextafter(np.float32(1), up)), (8.0, -4.0, np.nextafter(np.float32(-1), -up)))
    assert not R.inside(out, box).any()


def test_restatement_nan_and_inf_are_outside_and_bad_boxes_hold_nothing():
    box = [0.0, 0.0, 0.0, 1.0, 2.0, 2.0, 0.3]
    bad = np.float32([np.nan, np.inf, -np.inf])
    rows = [(0.0, 0.0, 0.5)]
    for v in bad:
        rows += [(v, 0.0, 0.5), (0.0, v, 0.5), (0.0, 0.0, v)]
    got = R.inside(_pt(*rows), box)
    assert got[0] and not got[1:].any()
    cloud = _pt((0.0, 0.0, 0.5), (0.1, -0.2, 0.3))
    good = list(R.entry(box))
    assert R.inside_entry(cloud, good).all()
    for field in range(8):
        e = list(good)
        e[field] = np.nan
        assert not R.inside_entry(cloud, e).any(), field
    e = list(good)
    e[4] = -1.0                                           # hl < 0
    assert not R.inside_entry(cloud, e).any()
    # index / counts / paste on a two-box toy: the shared point counts twice and belongs to the lower index
    boxes = [[0.0, 0.0, 0.0, 1.0, 2.0, 2.0, 0.0], [1.0, 0.0, 0.0, 1.0, 2.0, 2.0, 0.0]]
    cloud = _pt((-0.5, 0.0, 0.5), (0.5, 0.0, 0.5), (1.5, 0.0, 0.5), (5.0, 0.0, 0.5), (np.nan, 0.0, 0.5))
    index, counts = R.index_counts(cloud, boxes)
    assert index.tolist() == [0, 0, 1, -1, -1] and counts.tolist() == [2, 2]
    out, count = R.paste(cloud, boxes, _pt((7.0, 7.0, 7.0)), cap=4)
    assert count == 2 and np.array_equal(out[:2], np.concatenate([cloud[3:4], _pt((7.0, 7.0, 7.0))])) and np.isnan(out[2:]).all()


def test_box_table_is_the_restatements_entry(ref_db):
    from voxelnet_amd import gtsample as G
    boxes = np.array([e["box"] for e in ref_db])
    t = G.box_table(boxes)
    assert t.dtype == G.BOX_DTYPE and t.dtype.itemsize == 64 and t.shape == (96,)
    for row, box in zip(t, boxes):
        assert row.tobytes() == np.array(R.entry(box), dtype=np.float64).tobytes()
    assert G.box_table(np.zeros((0, 7))).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------------------------------
def _check_draw(db_ref, sampler, labels, tag, per_class, min_points=5):
    state = np.random.get_state()
    want = R.draw(db_ref, labels, tag, per_class, min_points)
    after_ref = np.random.get_state()
    np.random.set_state(state)
    got = sampler.draw(labels, tag)
    assert _same_state(np.random.get_state(), after_ref)
    assert got.lines == want["lines"]
    assert got.boxes.tobytes() == want["boxes"].tobytes() and got.boxes.shape == want["boxes"].shape
    assert got.points.dtype == np.float32 and got.points.tobytes() == want["points"].tobytes()
    assert got.table.shape == (len(want["lines"]),)
    for row, box in zip(got.table, want["boxes"]):
        assert row.tobytes() == np.array(R.entry(box), dtype=np.float64).tobytes()
    return got


def test_draw_matches_the_restatement_and_consumes_one_permutation(ref_db):
    from voxelnet_amd import gtsample as G
    assert len(ref_db) == 96 and sum(len(e["points"]) >= 5 for e in ref_db) == 55
    db = _package_db(ref_db)
    sampler = G.GTSampler(db, per_class={"Car": 15}, min_points=5)
    for f in range(4):
        _, labels = _frame(f)
        np.random.seed(100 + f)
        before = np.random.get_state()
        got = _check_draw(ref_db, sampler, labels, f"{f:06d}", {"Car": 15})
        after = np.random.get_state()
        np.random.set_state(before)
        np.random.permutation(55)                          # every pool entry has another tag: len(pool) == 55
        assert _same_state(np.random.get_state(), after)
        assert 5 <= len(got.lines) <= 9                    # want = 15 - 6 = 9 candidates
        # the re-parsed enlarged label gives the database boxes bit for bit
        from voxelnet_amd.targets import label_to_gt_box_3d
        again = label_to_gt_box_3d([list(labels) + got.lines], "", "lidar")[0]
        assert again[len(labels):].tobytes() == got.boxes.tobytes()
        # nothing accepted overlaps anything
        from augment_ref import overlap
        allb = list(again)
        assert not any(overlap(allb[i], allb[j]) for i in range(len(allb)) for j in range(len(labels), len(allb)) if i < j)


def test_draw_with_nothing_wanted_or_an_empty_pool_consumes_nothing(ref_db):
    from voxelnet_amd import gtsample as G
    db = _package_db(ref_db)
    _, labels = _frame(0)
    np.random.seed(5)
    before = np.random.get_state()
    for sampler in (G.GTSampler(db, per_class={"Car": 6}),                     # six cars are there already: want == 0
                    G.GTSampler(db, per_class={"Car": 3}),
                    G.GTSampler(db, per_class={"Pedestrian": 4}),              # no such entry: empty pool
                    G.GTSampler(db, per_class={"Car": 15}, min_points=10 ** 6),
                    G.GTSampler(G.GTDatabase([]), per_class={"Car": 15})):
        got = sampler.draw(labels, "000000")
        assert got.lines == [] and got.table.shape == (0,) and got.points.shape == (0, 4) and got.boxes.shape == (0, 7)
        assert _same_state(np.random.get_state(), before)


def test_draw_never_takes_the_frames_own_tag_or_small_objects(ref_db):
    from voxelnet_amd import gtsample as G
    db = _package_db(ref_db)
    own = "000012"
    sampler = G.GTSampler(db, per_class={"Car": 200}, min_points=12)
    big = [e for e in ref_db if len(e["points"]) >= 12]
    assert 0 < len(big) < 55 and any(e["tag"] == own for e in big)
    seen = []
    for seed in range(6):
        np.random.seed(seed)
        got = _check_draw(ref_db, sampler, [], own, {"Car": 200}, 12)
        seen += got.lines
    by_line = {e["line"]: e for e in ref_db}
    assert len(seen) >= 20
    assert all(by_line[line]["tag"] != own and len(by_line[line]["points"]) >= 12 for line in seen)
    # an empty frame with every candidate tried: whatever is left out collides with something taken, or is barred
    np.random.seed(0)
    got = sampler.draw([], own)
    from augment_ref import overlap
    for e in big:
        if e["tag"] != own and e["line"] not in got.lines:
            assert any(overlap(e["box"], b) for b in got.boxes)


def _entry(x, y, tag, cls="Car", n=6, r=0.0):
    from voxelnet_amd.targets import lidar_box_to_label_line
    line = lidar_box_to_label_line(cls, [x, y, -1.5, 1.5, 1.6, 4.0, r])
    return dict(cls=cls, tag=tag, box=R.line_box(line), points=np.full((n, 4), x, np.float32), line=line)


def test_draw_refuses_collisions_and_takes_a_later_disjoint_candidate():
    from voxelnet_amd import gtsample as G
    from voxelnet_amd.targets import lidar_box_to_label_line
    labels = [lidar_box_to_label_line("Car", [20.0, 0.0, -1.5, 1.5, 1.6, 4.0, 0.0])]
    # A overlaps the frame's car, B is free, C overlaps B, D is free
    ref = [_entry(21.0, 0.5, "a"), _entry(40.0, 10.0, "b"), _entry(41.0, 10.5, "c"), _entry(60.0, -20.0, "d")]
    sampler = G.GTSampler(_package_db(ref), per_class={"Car": 5})
    outcomes = set()
    for seed in range(40):
        np.random.seed(seed)
        order = np.random.permutation(4)
        np.random.seed(seed)
        got = _check_draw(ref, sampler, labels, "frame", {"Car": 5})
        tags = [{e["line"]: e["tag"] for e in ref}[line] for line in got.lines]
        first_bc = "b" if list(order).index(1) < list(order).index(2) else "c"
        assert tags == [ref[j]["tag"] for j in order if ref[j]["tag"] in (first_bc, "d")], (seed, order, tags)
        outcomes.add(tuple(tags))
    assert len(outcomes) >= 4                                # b before c and c before b, d early and late


def test_draw_stops_at_128_and_walks_the_classes_in_order():
    from voxelnet_amd import gtsample as G
    # 150 disjoint cars on a 10 m lattice, 20 disjoint pedestrians beside them
    cars = [_entry(10.0 * (i % 15), 10.0 * (i // 15) - 45.0, f"c{i}") for i in range(150)]
    peds = [_entry(10.0 * i, 80.0, f"p{i}", cls="Pedestrian") for i in range(20)]
    ref = cars + peds
    db = _package_db(ref)
    np.random.seed(1)
    got = _check_draw(ref, G.GTSampler(db, per_class={"Car": 150}), [], "frame", {"Car": 150})
    assert len(got.lines) == 128 and got.table.shape == (128,) and got.points.shape == (128 * 6, 4)
    # two classes: per_class order decides both the order of the permutations and the order of the table
    for per_class in ({"Car": 4, "Pedestrian": 3}, {"Pedestrian": 3, "Car": 4}):
        np.random.seed(2)
        before = np.random.get_state()
        got = _check_draw(ref, G.GTSampler(db, per_class=per_class), [], "frame", per_class)
        after = np.random.get_state()
        kinds = [line.split()[0] for line in got.lines]
        first, second = list(per_class)
        assert kinds == [first] * per_class[first] + [second] * per_class[second]
        np.random.set_state(before)
        np.random.permutation(150 if first == "Car" else 20)
        np.random.permutation(20 if first == "Car" else 150)
        assert _same_state(np.random.get_state(), after)
    # the cap holds across classes, and a class drawn at the cap still consumes its permutation (the rule has no exception)
    np.random.seed(3)
    got = _check_draw(ref, G.GTSampler(db, per_class={"Car": 150, "Pedestrian": 5}), [], "frame", {"Car": 150, "Pedestrian": 5})
    assert len(got.lines) == 128 and all(line.split()[0] == "Car" for line in got.lines)


def test_database_save_load_round_trip(tmp_path, ref_db):
    from voxelnet_amd import gtsample as G
    ref = list(ref_db[:20]) + [_entry(5.0, 5.0, "own", cls="Pedestrian", n=0)]
    ref[3] = dict(ref[3], line=ref[3]["line"] + "\n")          # a line as readlines() gives it
    db = _package_db(ref)
    path = str(tmp_path / "db.npz")
    db.save(path)
    back = G.GTDatabase.load(path)
    assert len(back) == len(db) == 21
    for a, b in zip(db.entries, back.entries):
        assert (a.cls, a.tag, a.line) == (b.cls, b.tag, b.line)
        assert a.box.tobytes() == b.box.tobytes() and b.box.dtype == np.float64
        assert a.points.tobytes() == b.points.tobytes() and b.points.dtype == np.float32 and a.points.shape == b.points.shape
    assert back.entries[-1].points.shape == (0, 4) and back.entries[3].line.endswith("\n")
    empty = str(tmp_path / "empty.npz")
    G.GTDatabase([]).save(empty)
    assert len(G.GTDatabase.load(empty)) == 0


def test_no_cpu_path_for_the_points():
    import torch
    from voxelnet_amd import _lib
    from voxelnet_amd import gtsample as G
    cloud = torch.zeros((8, 4))
    params = G.GTSampleParams(G.box_table(np.zeros((0, 7))), np.zeros((0, 4), np.float32), np.zeros((0, 7)), [])
    with pytest.raises(_lib.VoxelnetHipError):
        G.points_in_boxes_device(cloud, G.box_table(np.zeros((1, 7))))
    with pytest.raises(_lib.VoxelnetHipError):
        G.gt_paste_device(cloud, params)
    with pytest.raises(_lib.VoxelnetHipError):
        G.enqueue_gt_paste(cloud, params)
    with pytest.raises(_lib.VoxelnetHipError):
        G.GTDatabase.build([("t", np.zeros((4, 4), np.float32), [])], device="cpu")
    assert _lib.VN_GT_MAX_BOXES == G.MAX_BOXES == 128
    # the table's three descriptions agree: NumPy dtype, ctypes structure, eight float64 fields in the header's order
    import ctypes
    assert ctypes.sizeof(_lib.VnGtBox) == 64 and [f for f, _ in _lib.VnGtBox._fields_] == list(G.BOX_DTYPE.names)
    assert [getattr(_lib.VnGtBox, f).offset for f in G.BOX_DTYPE.names] == [G.BOX_DTYPE.fields[f][1] for f in G.BOX_DTYPE.names]


def test_entry_points_check_their_arguments_on_the_host():
    """status codes of the two entry points that need no device work to decide (the conventions of vn_fov_crop)"""
    import ctypes
    from voxelnet_amd import _lib
    lib = _lib.load()
    assert lib.vn_gt_paste_workspace_bytes(-1) == 0 and lib.vn_gt_paste_workspace_bytes(1 << 31) == 0
    assert lib.vn_gt_paste_workspace_bytes(0) > 0
    assert lib.vn_gt_paste_workspace_bytes(20000) >= 20000 + 4 * (79 + 1)
    ws = lib.vn_gt_paste_workspace_bytes(1000)
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16
    E, U, W = -1, -2, -3
    paste = lib.vn_gt_paste
    assert paste(0x1000, 1000, None, 0, 0x10000, 10, 0x100000, 1009, a, a, ws, None) == E          # cap < n + m
    assert paste(0x1000, -1, None, 0, None, 0, 0x100000, 10, a, a, ws, None) == E
    assert paste(0x1000, 1000, None, 129, None, 0, 0x100000, 1000, a, a, ws, None) == E
    assert paste(0x1000, 1000, None, 1, None, 0, 0x100000, 1000, a, a, ws, None) == E              # a table without a pointer
    assert paste(0x1000, 1000, None, 0, None, 0, 0x100000, 1000, None, a, ws, None) == E           # no count
    assert paste(0x1000, 1000, None, 0, None, 0, 0x2000, 1000, a, a, ws, None) == E                # out overlaps the scene
    assert paste(0x1000, 1000, None, 0, 0x100100, 10, 0x100000, 1010, a, a, ws, None) == E         # out overlaps the objects
    assert paste(0x1000, 1000, None, 0, None, 0, 0x100000, 1000, a, a, ws - 1, None) == W
    assert paste(0x1004, 1000, None, 0, None, 0, 0x100000, 1000, a, a, ws, None) == U              # 4-byte-offset pointers
    assert paste(0x1000, 1000, None, 0, None, 0, 0x100004, 1000, a, a, ws, None) == U
    assert paste(0x1000, 1000, None, 0, 0x10004, 10, 0x100000, 1010, a, a, ws, None) == U
    assert paste(0x1000, 1000, 0x20008, 3, None, 0, 0x100000, 1000, a, a, ws, None) == U
    pib = lib.vn_points_in_boxes
    assert pib(0x1000, -1, None, 0, 0x2000, None, None) == E
    assert pib(0x1000, 10, None, 129, 0x2000, None, None) == E
    assert pib(0x1000, 10, None, 2, 0x2000, None, None) == E
    assert pib(None, 10, None, 0, 0x2000, None, None) == E
    assert pib(0x1000, 10, None, 0, None, None, None) == E
    assert pib(0x1004, 10, None, 0, 0x2000, None, None) == U
    assert pib(0x1000, 10, 0x3008, 2, 0x2000, None, None) == U
    assert pib(None, 0, None, 0, None, None, None) == 0                                             # n == 0, no counts: a no-op
