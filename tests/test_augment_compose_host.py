"""CPU: the host half of the composed augmentation (voxelnet_amd/augment.py: ComposeRecipe, draw_compose,
compose_labels) — the order in which the draw consumes np.random, the collision rule of the object noise, the label round
trip — and the argument checks and struct layouts of `vn_augment_compose`.  The per-point work has no CPU path:
tests/test_gpu_augment_compose.py checks it on the device against tests/compose_ref.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import compose_ref as R


def _labels(seed=0, n=6):
    from voxelnet_amd import synth
    return synth.synth_labels("Car", n, seed)


def _line(cls, x, y, z, h, w, l, r):
    from voxelnet_amd.targets import lidar_box_to_label_line
    return lidar_box_to_label_line(cls, [x, y, z, h, w, l, r])


ONE = ["Car 0 0 0 0 0 0 0 1.5 1.6 3.9 -8.0 1.6 12.0 0.3"]          # ONE box: nothing to collide with, first candidate taken


def test_draw_consumes_the_stream_in_the_stated_order():
    """a hand-written replay of the five stages reproduces every parameter and leaves np.random at the same place"""
    from voxelnet_amd import augment as A
    rec = A.ComposeRecipe(translate_sigma=(0.2, 0.3, 0.1))
    np.random.seed(3)
    p = A.draw_compose(ONE, rec)
    tail = np.random.random()
    np.random.seed(3)
    rz = np.random.uniform(-np.pi / 4, np.pi / 4)
    tx, ty, tz = np.random.normal() * 1.0, np.random.normal() * 1.0, np.random.normal() * 0.5
    flip = np.random.random() < 0.5
    angle = np.random.uniform(-np.pi / 4, np.pi / 4)
    factor = np.random.uniform(0.95, 1.05)
    t = (np.random.normal() * 0.2, np.random.normal() * 0.3, np.random.normal() * 0.1)
    assert np.random.random() == tail
    row = p.table[0]
    assert len(p.table) == 1 and p.entry_line == [0]
    assert (row["tx"], row["ty"], row["tz"], row["rc"], row["rs"]) == (tx, ty, tz, np.cos(rz), np.sin(rz))
    assert (p.flip_y, p.angle, p.factor, tuple(p.translate)) == (bool(flip), angle, factor, t)
    # the table holds the UNMOVED box in vnGtBox's fields
    b = p.boxes_before[0]
    assert (row["x"], row["y"], row["z0"], row["z1"], row["hl"], row["hw"], row["c"], row["s"]) == \
        (b[0], b[1], b[2], b[2] + b[3], b[5] / 2, b[4] / 2, np.cos(b[6]), np.sin(b[6]))
    # the moved box, stage by stage
    from voxelnet_amd.targets import _limit_angle
    x, y, z, r = b[0] + tx, b[1] + ty, b[2] + tz, _limit_angle(b[6] + rz)
    if flip:
        y, r = -y, -r
    c, s = np.cos(angle), np.sin(angle)
    x, y, r = x * c + y * s, -(x * s) + y * c, r - angle
    want = np.array([x, y, z, b[3], b[4], b[5], r])
    want[0:6] *= factor
    want[0:3] += np.array(t)
    assert np.array_equal(p.boxes_after[0], want)
    # the eight numbers of the affine
    fy, f = (-1.0 if flip else 1.0), float(np.float32(factor))
    assert np.array_equal(p.affine, np.array([f * c, f * (s * fy), f * (-s), f * (c * fy), f, t[0], t[1], t[2]]))


def test_a_disabled_stage_consumes_nothing():
    from voxelnet_amd import augment as A
    off = dict(object_rot=None, object_sigma=None, flip=None, rotation=None, scale=None, translate_sigma=None)
    np.random.seed(11)
    first = np.random.random()
    np.random.seed(11)
    p = A.draw_compose(_labels(), A.ComposeRecipe(**off))
    assert np.random.random() == first                                   # everything off: not one number drawn
    assert len(p.table) == 0 and np.array_equal(p.boxes_after, p.boxes_before)
    assert np.array_equal(p.affine, [1, 0, 0, 1, 1, 0, 0, 0])
    # one stage on at a time: exactly that stage's numbers
    draws = {"flip": (dict(flip=0.5), lambda: np.random.random()),
             "rotation": (dict(rotation=0.3), lambda: np.random.uniform(-0.3, 0.3)),
             "scale": (dict(scale=(0.9, 1.1)), lambda: np.random.uniform(0.9, 1.1)),
             "translate": (dict(translate_sigma=(1, 1, 1)), lambda: [np.random.normal() for _ in range(3)]),
             "noise": (dict(object_rot=0.1, object_sigma=(1, 1, 1)), lambda: [np.random.uniform(-0.1, 0.1)] + [np.random.normal() for _ in range(3)]),
             "attempts 0": (dict(object_rot=0.1, object_sigma=(1, 1, 1), attempts=0), lambda: None),
             "flip 0": (dict(flip=0), lambda: None)}
    for name, (kw, replay) in draws.items():
        np.random.seed(12)
        A.draw_compose(ONE, A.ComposeRecipe(**{**off, **kw}))
        tail = np.random.random()
        np.random.seed(12)
        replay()
        assert np.random.random() == tail, name


def test_draw_equals_the_restatement_over_200_seeds():
    from voxelnet_amd import augment as A
    recipes = [{}, dict(translate_sigma=(0.2, 0.2, 0.1)), dict(flip=None, scale=None), dict(object_rot=None, object_sigma=None),
               dict(attempts=3, object_sigma=(4.0, 4.0, 0.5))]
    placed = 0
    for seed in range(200):
        labels = _labels(seed % 7, 3 + seed % 9)
        kw = recipes[seed % len(recipes)]
        np.random.seed(seed)
        p = A.draw_compose(labels, A.ComposeRecipe(**kw))
        tail = np.random.random()
        np.random.seed(seed)
        d = R.draw(labels, R.recipe(**kw))
        assert np.random.random() == tail, seed
        assert R.same_draw(p, d), seed
        placed += len(p.table)
    assert placed > 500


def _crowded(rng, n=12):
    """n cars in a 20 m x 12 m lot, pairwise non-overlapping (rejection sampling)"""
    from voxelnet_amd import augment as A
    from voxelnet_amd.targets import label_to_gt_box_3d
    lines = []
    while len(lines) < n:
        cand = _line("Car", 20 + rng.uniform(0, 20), rng.uniform(-6, 6), -1.7, 1.5, 1.6, 3.9, rng.uniform(-1.5, 1.5))
        boxes = label_to_gt_box_3d([lines + [cand]], "", "lidar")[0]
        if not any(A.footprints_overlap(boxes[-1], b) for b in boxes[:-1]):
            lines.append(cand)
    return lines


def test_accepted_boxes_are_pairwise_non_overlapping():
    """crowded frames whose original boxes do not overlap: after the object noise no two boxes overlap, whether they
    moved or stayed — each candidate was tested against EVERY other box in its current state"""
    from voxelnet_amd import augment as A
    rng = np.random.default_rng(4)
    only_noise = A.ComposeRecipe(flip=None, rotation=None, scale=None)
    retried = 0
    for frame in range(30):
        labels = _crowded(rng) + ["DontCare -1 -1 -10 0 0 0 0 -1 -1 -1 -1000 -1000 -1000 -10"]
        np.random.seed(frame)
        p = A.draw_compose(labels, only_noise)
        n = 12
        for i in range(n):
            for j in range(i):
                assert not A.footprints_overlap(p.boxes_after[i], p.boxes_after[j]), (frame, i, j)
        assert p.entry_line == [i for i in range(n) if not np.array_equal(p.boxes_after[i], p.boxes_before[i])]
        assert np.array_equal(p.boxes_after[n], p.boxes_before[n]) and not p.has_box[n]
        # np.random stands at the start: did some accepted move differ from the first candidate drawn for its box?
        np.random.seed(frame)
        for i in range(n):
            np.random.uniform(-np.pi / 4, np.pi / 4)
            t = (np.random.normal(), np.random.normal(), np.random.normal() * 0.5)
            if i >= len(p.table) or (p.table[i]["tx"], p.table[i]["ty"], p.table[i]["tz"]) != t:
                retried += 1
                break
    assert retried > 0          # some first candidate collided somewhere: the rule was exercised, not vacuous


def test_a_box_that_cannot_be_placed_stays_and_gets_no_entry():
    """box 0 has a 400 m x 400 m footprint: every candidate of box 1 (moved by a few metres) lands inside it, so box 1
    stays where it was after `attempts` tries and gets no table entry; box 0 itself cannot move either (box 1 is inside
    it wherever it goes); box 2, far outside, moves.  The stream consumed 4 numbers per attempt: 7 + 7 + 1 attempts."""
    from voxelnet_amd import augment as A
    labels = [_line("Car", 30.0, 0.0, -1.7, 1.5, 400.0, 400.0, 0.2), _line("Car", 35.0, 3.0, -1.7, 1.5, 1.6, 3.9, 0.1),
              _line("Car", 900.0, 900.0, -1.7, 1.5, 1.6, 3.9, 0.1)]
    rec = A.ComposeRecipe(attempts=7, flip=None, rotation=None, scale=None)
    np.random.seed(2)
    p = A.draw_compose(labels, rec)
    tail = np.random.random()
    assert p.entry_line == [2] and len(p.table) == 1
    assert np.array_equal(p.boxes_after[:2], p.boxes_before[:2]) and not np.array_equal(p.boxes_after[2], p.boxes_before[2])
    assert p.table[0]["x"] == p.boxes_before[2, 0]
    np.random.seed(2)
    for _ in range(7 + 7 + 1):
        np.random.uniform(-np.pi / 4, np.pi / 4)
        np.random.normal(), np.random.normal(), np.random.normal()
    assert np.random.random() == tail


def test_flip_is_drawn_for_half_of_2000_seeds():
    """0.5 +- 0.05 of 2,000 seeds: 4.5 standard deviations of the binomial (sqrt(0.25 / 2000) = 0.0112)"""
    from voxelnet_amd import augment as A
    rec = A.ComposeRecipe(object_rot=None, object_sigma=None)
    flips = 0
    for seed in range(2000):
        np.random.seed(20_000 + seed)
        flips += A.draw_compose(ONE, rec).flip_y
    assert abs(flips / 2000 - 0.5) <= 0.05, flips


def test_the_object_turn_moves_the_long_axis_with_the_points():
    """r' = r + rz: points on the long axis of the unmoved box, moved by the table entry's formulas (float64, host), lie on
    the long axis of the moved box — checked through gtsample.box_table's c, s of the moved box, with no device"""
    from voxelnet_amd import augment as A
    from voxelnet_amd import gtsample as G
    rec = A.ComposeRecipe(flip=None, rotation=None, scale=None)
    for seed in range(20):
        np.random.seed(seed)
        p = A.draw_compose(ONE, rec)
        e, b0 = p.table[0], p.boxes_before[0]
        moved = G.box_table(p.boxes_after[:1])[0]
        for along in (-1.9, 0.7, 1.9):
            px, py = b0[0] + along * np.cos(b0[6]), b0[1] + along * np.sin(b0[6])          # on the long axis, in the box
            dx, dy = px - e["x"], py - e["y"]
            X = (e["x"] + e["tx"]) + (dx * e["rc"] - dy * e["rs"])
            Y = (e["y"] + e["ty"]) + (dx * e["rs"] + dy * e["rc"])
            u = (X - moved["x"]) * moved["c"] + (Y - moved["y"]) * moved["s"]
            v = -((X - moved["x"]) * moved["s"]) + (Y - moved["y"]) * moved["c"]
            assert abs(abs(u) - abs(along)) < 1e-9 and abs(v) < 1e-9, (seed, along, u, v)          # (|u|: r is kept modulo pi)


def test_compose_labels_round_trip_within_the_two_decimal_format():
    """compose_labels -> label_to_gt_box_3d gives the moved boxes back within what two decimals can hold (the bounds of
    tests/test_augment_host.py's round trip: 0.005 per printed field, stretched by the inverse calibration for the centre;
    the angle modulo pi, with _limit_angle's 5-degree snap above -pi/2); DontCare lines pass through verbatim"""
    from voxelnet_amd import augment as A
    from voxelnet_amd import targets as T
    half = 0.005
    lin = np.matmul(T._T_VELO_2_CAM_INV, T._R_RECT_0_INV)[:3, :3]
    pos_bound = np.linalg.norm(lin, 2) * half * np.sqrt(3) + 1e-9
    snap = 5 / 180 * np.pi
    for seed in range(60):
        labels = _labels(seed, 6)
        np.random.seed(seed)
        p = A.draw_compose(labels, A.ComposeRecipe(translate_sigma=(0.2, 0.2, 0.1)))
        lines = A.compose_labels(labels, p)
        assert len(lines) == len(labels) and [l.split()[0] for l in lines] == [l.split()[0] for l in labels]
        assert lines[6] == labels[6] and labels[6].startswith("DontCare") and not p.has_box[6]          # verbatim
        assert np.array_equal(p.boxes_after[6], p.boxes_before[6])
        back = T.label_to_gt_box_3d([lines], "", "lidar")[0][:6]
        after = p.boxes_after[:6]
        assert np.abs(back[:, :3] - after[:, :3]).max() <= pos_bound, seed
        assert np.abs(back[:, 3:6] - after[:, 3:6]).max() <= half + 1e-9, seed
        for r0, r1 in zip(after[:, 6], back[:, 6]):
            d = abs((r1 - r0 + np.pi / 2) % np.pi - np.pi / 2)                # circular distance modulo pi
            in_snap_zone = abs((r0 + np.pi / 2) % np.pi) < snap + half or abs((r0 + np.pi / 2) % np.pi - np.pi) < half
            assert d <= half + 1e-9 or (in_snap_zone and d <= snap + half + 1e-9), (seed, r0, r1)
    with pytest.raises(ValueError):
        A.compose_labels(labels[:-1], p)


def test_more_than_128_accepted_moves_raise():
    from voxelnet_amd import _lib
    from voxelnet_amd import augment as A
    labels = [_line("Car", 10.0 * (i % 13), 10.0 * (i // 13) - 50, -1.7, 1.5, 1.6, 3.9, 0.1) for i in range(A.MAX_BOXES + 1)]
    np.random.seed(0)
    with pytest.raises(_lib.VoxelnetHipError):
        A.draw_compose(labels, A.ComposeRecipe(object_sigma=(0.1, 0.1, 0.1)))
    np.random.seed(0)
    assert len(A.draw_compose(labels[:-1], A.ComposeRecipe(object_sigma=(0.1, 0.1, 0.1))).table) == A.MAX_BOXES


def test_vn_augment_compose_argument_checks():
    """the stated status codes; every check runs before any launch, so none of these calls needs a GPU"""
    from voxelnet_amd import _lib
    lib = _lib.load()
    f = lib.vn_augment_compose
    aff = _lib.VnAffine(1, 0, 0, 1, 1, 0, 0, 0)
    a = ctypes.byref(aff)
    ok, bad = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    assert f(None, 0, None, 0, a, None, None) == 0                                   # n == 0: a no-op
    assert f(None, 0, ok, _lib.VN_AUGMENT_MAX_BOXES, a, None, None) == 0
    assert f(None, -1, None, 0, a, None, None) == -1
    assert f(ok, 1 << 31, None, 0, a, ok, None) == -1
    assert f(None, 0, None, -1, a, None, None) == -1
    assert f(None, 0, ok, _lib.VN_AUGMENT_MAX_BOXES + 1, a, None, None) == -1
    assert f(None, 0, None, 0, None, None, None) == -1                               # NULL affine
    assert f(ok, 10, None, 0, None, ok, None) == -1
    assert f(None, 0, None, 2, a, None, None) == -1                                  # NULL moves with n_moves > 0
    assert f(ok, 10, None, 2, a, ok, None) == -1
    assert f(None, 10, None, 0, a, ok, None) == -1                                   # NULL points / out with n > 0
    assert f(ok, 10, None, 0, a, None, None) == -1
    assert f(bad, 10, None, 0, a, ok, None) == -2                                    # misaligned pointers
    assert f(ok, 10, None, 0, a, bad, None) == -2
    assert f(ok, 10, ctypes.c_void_p(4104), 2, a, ok, None) == -2
    assert _lib.ABI_VERSION == lib.vn_abi_version() == 4                             # the symbol is additive


def test_both_structs_match_the_header_layout(tmp_path):
    """vnObjectMove / vnAffine: the C header, the ctypes structures and the NumPy record the table is staged from agree on
    size and on every field offset; vnObjectMove begins with vnGtBox's eight fields"""
    from voxelnet_amd import _lib
    from voxelnet_amd import augment as A
    from voxelnet_amd import gtsample as G
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    move = ["x", "y", "z0", "z1", "hl", "hw", "c", "s", "tx", "ty", "tz", "rc", "rs", "pad"]
    aff = ["a00", "a01", "a10", "a11", "sz", "bx", "by", "bz"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "voxelnet_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vnObjectMove));\n'
                   + "".join(f'  printf(" %zu", offsetof(vnObjectMove, {n}));\n' for n in move)
                   + '  printf("\\n%zu", sizeof(vnAffine));\n'
                   + "".join(f'  printf(" %zu", offsetof(vnAffine, {n}));\n' for n in aff)
                   + '  printf("\\n%zu", sizeof(vnGtBox));\n'
                   + "".join(f'  printf(" %zu", offsetof(vnGtBox, {n}));\n' for n in move[:8])
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    got_move, got_aff, got_gt = ([int(v) for v in line.split()] for line in out)
    assert got_move == [128] + [8 * i for i in range(14)]
    assert got_move == [ctypes.sizeof(_lib.VnObjectMove)] + [getattr(_lib.VnObjectMove, n).offset for n in move]
    assert got_move == [A.MOVE_DTYPE.itemsize] + [A.MOVE_DTYPE.fields[n][1] for n in move]
    assert got_aff == [64] + [8 * i for i in range(8)]
    assert got_aff == [ctypes.sizeof(_lib.VnAffine)] + [getattr(_lib.VnAffine, n).offset for n in aff]
    assert list(A.AFFINE_FIELDS) == aff
    assert got_gt[1:] == got_move[1:9] and [G.BOX_DTYPE.fields[n][1] for n in move[:8]] == got_move[1:9]


def test_points_have_no_cpu_path():
    import torch
    from voxelnet_amd import _lib
    from voxelnet_amd import augment as A
    np.random.seed(0)
    p = A.draw_compose(_labels(), A.ComposeRecipe())
    with pytest.raises(_lib.VoxelnetHipError):
        A.compose_points_device(torch.zeros(8, 4), p)
    with pytest.raises(_lib.VoxelnetHipError):
        A.compose_points_device(np.zeros((8, 4), np.float32), p)
    with pytest.raises(_lib.VoxelnetHipError):
        A.enqueue_compose_points(torch.zeros(8, 4), p)


def test_unknown_augment_values_raise(monkeypatch):
    """`augment` is True, False or a ComposeRecipe instance; the check comes before anything touches the device"""
    from voxelnet_amd import augment as A
    from voxelnet_amd import dataset as D
    monkeypatch.setattr(D, "pipeline_stream", lambda device: None)
    for bad in ("second", "compose", 1, 0, None, A.ComposeRecipe, {"flip": 0.5}):
        with pytest.raises(ValueError, match="augment"):
            D.DeviceCollate("cuda:0", "Car", augment=bad)
        with pytest.raises(ValueError, match="augment"):
            D.DeviceBatcher([], "cuda:0", "Car", augment=bad)
    for good in (True, False, np.bool_(True), A.ComposeRecipe(), A.ComposeRecipe(flip=None)):
        c = D.DeviceCollate("cuda:0", "Car", augment=good)
        is_recipe = isinstance(good, A.ComposeRecipe)
        assert (c.recipe is good) == is_recipe and c.augment == (not is_recipe and bool(good))


def test_frames_hold_points_inside_the_cars_and_the_margin_leaves_out_few():
    """the frames tests/test_gpu_augment_compose.py moves on the device (compose_ref.frame(0..3), and 8..13 for its
    database), with the restatement alone: 6,000 points, no exact zero, every car holds >= 40 points, and at most 2 % of a
    frame's in-box points lie within 1e-3 m of a face (what the rigidity test there may leave out)"""
    for f in list(range(4)) + list(range(8, 14)):
        cloud, labels = R.frame(f)
        assert cloud.shape == (6000, 4) and cloud.dtype == np.float32 and not (cloud[:, :3] == 0).any()
        boxes = R.label_to_gt_box_3d([labels], "", "lidar")[0]
        table = [R.entry(b, 0.0, 0.0, 0.0, 0.0) for b in boxes[:6]]
        counts = [int(R.inside(cloud, e).sum()) for e in table]
        assert min(counts) >= 40 and int(R.inside(cloud, R.entry(boxes[6], 0, 0, 0, 0)).sum()) == 0, (f, counts)
        if f < 4:
            near = 0
            for e in table:
                shrunk = dict(e, hl=e["hl"] - 1e-3, hw=e["hw"] - 1e-3, z0=e["z0"] + 1e-3, z1=e["z1"] - 1e-3)
                near += int((R.inside(cloud, e) & ~R.inside(cloud, shrunk)).sum())
            assert near <= 0.02 * sum(counts), (f, near, counts)
