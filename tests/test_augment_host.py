"""CPU: the host half of the device-side augmentation (voxelnet_amd/augment.py; the reference's pcl_augmentation,
voxelnet/dataset.py:122-219) — the order in which the draw consumes np.random, the 3 / 3 / 4 mode split, the collision
rule of the box perturbation, the label round trip — and the argument checks of `vn_augment_points`.  The per-point work
has no CPU path: tests/test_gpu_augment.py checks it on the device against tests/augment_ref.py."""
import ctypes
import subprocess

import numpy as np
import pytest

import augment_ref as R


def _labels(seed=0, n=6):
    from voxelnet_amd import synth
    return synth.synth_labels("Car", n, seed)


def _line(cls, x, y, z, h, w, l, r):
    from voxelnet_amd.targets import lidar_box_to_label_line
    return lidar_box_to_label_line(cls, [x, y, z, h, w, l, r])


def _seed_with_choice(pred, start=0):
    for seed in range(start, start + 1000):
        np.random.seed(seed)
        if pred(np.random.randint(0, 10)):
            return seed
    raise AssertionError("no seed found")


def test_draw_consumes_the_stream_in_the_specified_order():
    """a hand-written replay of the specification's draw order reproduces mode and parameters, for each of the three modes"""
    from voxelnet_amd import augment as A
    labels = ["Car 0 0 0 0 0 0 0 1.5 1.6 3.9 -8.0 1.6 12.0 0.3"]          # ONE box: nothing to collide with, first attempt taken
    # scale
    seed = _seed_with_choice(lambda c: c < 4)
    np.random.seed(seed)
    p = A.draw_augmentation(labels)
    np.random.seed(seed)
    choice, factor = np.random.randint(0, 10), np.random.uniform(0.95, 1.05)
    after = np.random.random()
    assert (p.mode, p.choice, p.factor) == ("scale", choice, factor)
    np.random.seed(seed)
    A.draw_augmentation(labels)
    assert np.random.random() == after                                   # nothing more was consumed
    assert np.array_equal(p.boxes_after[:, :6], p.boxes_before[:, :6] * factor) and p.boxes_after[0, 6] == p.boxes_before[0, 6]
    # rotate
    seed = _seed_with_choice(lambda c: 4 <= c < 7)
    np.random.seed(seed)
    p = A.draw_augmentation(labels)
    np.random.seed(seed)
    choice, angle = np.random.randint(0, 10), np.random.uniform(-np.pi / 4, np.pi / 4)
    after = np.random.random()
    assert (p.mode, p.choice, p.angle) == ("rotate", choice, angle)
    np.random.seed(seed)
    A.draw_augmentation(labels)
    assert np.random.random() == after
    x, y = p.boxes_before[0, 0], p.boxes_before[0, 1]
    c, s = np.cos(angle), np.sin(angle)
    assert p.boxes_after[0, 0] == x * c + y * s and p.boxes_after[0, 1] == -(x * s) + y * c
    assert np.array_equal(p.boxes_after[0, 2:6], p.boxes_before[0, 2:6])
    # boxes: rz, then tx, ty, tz
    seed = _seed_with_choice(lambda c: c >= 7)
    np.random.seed(seed)
    p = A.draw_augmentation(labels)
    np.random.seed(seed)
    choice, rz = np.random.randint(0, 10), np.random.uniform(-np.pi / 10, np.pi / 10)
    tx, ty, tz = np.random.normal(), np.random.normal(), np.random.normal()
    after = np.random.random()
    assert (p.mode, p.choice, len(p.table)) == ("boxes", choice, 1)
    row = p.table[0]
    assert tuple(row["t"]) == (tx, ty, tz) and row["c"] == np.cos(rz) and row["s"] == np.sin(rz)
    np.random.seed(seed)
    A.draw_augmentation(labels)
    assert np.random.random() == after
    b = p.boxes_before[0]
    X, Y = b[0] + tx, b[1] + ty
    assert p.boxes_after[0, 0] == X * np.cos(rz) + Y * np.sin(rz) and p.boxes_after[0, 1] == -(X * np.sin(rz)) + Y * np.cos(rz)
    assert p.boxes_after[0, 2] == b[2] + tz
    # bounds: hull of the UNMOVED box, float32, z from the bottom to bottom + h
    from voxelnet_amd.targets import gt_standup_boxes
    su = gt_standup_boxes(b.reshape(1, 7))[0]
    assert row["lo"].dtype == np.float32 and tuple(row["lo"]) == (su[0], su[1], np.float32(b[2]))
    assert tuple(row["hi"]) == (su[2], su[3], np.float32(b[2] + b[3]))


def test_draw_equals_the_restatement_over_many_seeds():
    """voxelnet_amd.augment.draw_augmentation and tests/augment_ref.draw (written separately, a different collision
    formulation) agree on every field and leave the np.random stream at the same place"""
    from voxelnet_amd import augment as A
    for seed in range(300):
        labels = _labels(seed % 7, 3 + seed % 9)
        np.random.seed(seed)
        p = A.draw_augmentation(labels)
        tail = np.random.random()
        np.random.seed(seed)
        d = R.draw(labels)
        assert np.random.random() == tail, seed
        assert (p.mode, p.choice) == (d["mode"], d["choice"]), seed
        assert np.array_equal(p.boxes_before, d["before"]) and np.array_equal(p.boxes_after, d["after"]), seed
        if p.mode == "boxes":
            assert len(p.table) == len(d["table"]), seed
            for row, (lo, hi, tx, ty, tz, c, s) in zip(p.table, d["table"]):
                assert np.array_equal(row["lo"], lo) and np.array_equal(row["hi"], hi), seed
                assert (tuple(row["t"]), row["c"], row["s"]) == ((tx, ty, tz), c, s), seed
        elif p.mode == "rotate":
            assert p.angle == d["angle"]
        else:
            assert p.factor == d["factor"]


def test_mode_frequencies_are_4_3_3_in_10():
    """2,000 seeds: scale (choice < 4), rotate (4..6), boxes (>= 7) appear with p = 0.4 / 0.3 / 0.3.  Bound: five
    standard deviations of a binomial count, sqrt(n p (1 - p)) — the seeds are independent draws of one uniform digit."""
    from voxelnet_amd import augment as A
    labels = _labels(1, 2)
    n = 2000
    counts = {"scale": 0, "rotate": 0, "boxes": 0}
    for seed in range(n):
        np.random.seed(10_000 + seed)
        counts[A.draw_augmentation(labels).mode] += 1
    for mode, prob in (("scale", 0.4), ("rotate", 0.3), ("boxes", 0.3)):
        assert abs(counts[mode] - n * prob) <= 5 * np.sqrt(n * prob * (1 - prob)), counts


def test_accepted_boxes_never_overlap_an_earlier_box():
    """crowded frames (12 cars in a 20 m x 12 m lot): whatever was accepted overlaps no earlier box in its moved state,
    by the package's test and by the restatement's; rejected boxes keep their place"""
    from voxelnet_amd import augment as A
    rng = np.random.default_rng(4)
    seen_retry = 0
    for frame in range(40):
        labels = [_line("Car", 20 + rng.uniform(0, 20), rng.uniform(-6, 6), -1.7, 1.5, 1.6, 3.9, rng.uniform(-1.5, 1.5)) for _ in range(12)]
        seed = _seed_with_choice(lambda c: c >= 7, start=1000 * frame)
        np.random.seed(seed)
        p = A.draw_augmentation(labels)
        assert p.mode == "boxes"
        moved = [i for i in range(12) if not np.array_equal(p.boxes_after[i], p.boxes_before[i])]
        assert len(moved) == len(p.table)
        for i in moved:
            for j in range(i):
                assert not A.footprints_overlap(p.boxes_after[i], p.boxes_after[j]), (frame, i, j)
                assert not R.overlap(p.boxes_after[i], p.boxes_after[j]), (frame, i, j)
        np.random.seed(seed)
        np.random.randint(0, 10)
        seen_retry += _first_attempts_collide(p)
    assert seen_retry > 0           # some first attempt collided somewhere: the rule was exercised, not vacuous


def _first_attempts_collide(p):
    """np.random stands right behind `choice`: True when the accepted motion of some box is not the first one drawn for
    it (a frame without any rejection consumes exactly one attempt = 4 numbers per box)"""
    for i in range(p.boxes_before.shape[0]):
        rz = np.random.uniform(-np.pi / 10, np.pi / 10)
        t = (np.random.normal(), np.random.normal(), np.random.normal())
        if i >= len(p.table) or tuple(p.table[i]["t"]) != t or p.table[i]["c"] != np.cos(rz):
            return True
    return False


def test_a_box_that_cannot_be_placed_stays_after_100_attempts():
    """box 0 has a 400 m x 400 m footprint: every candidate of box 1 (moved by a few metres) lands inside it, so box 1
    collides 100 times, stays where it was, gets no table entry, and the stream has consumed exactly 4 numbers per
    attempt: 4 (box 0) + 400 (box 1) + 4 (box 2, far outside)"""
    from voxelnet_amd import augment as A
    labels = [_line("Car", 30.0, 0.0, -1.7, 1.5, 400.0, 400.0, 0.2), _line("Car", 35.0, 3.0, -1.7, 1.5, 1.6, 3.9, 0.1),
              _line("Car", 900.0, 900.0, -1.7, 1.5, 1.6, 3.9, 0.1)]
    seed = _seed_with_choice(lambda c: c >= 7)
    np.random.seed(seed)
    p = A.draw_augmentation(labels)
    tail = np.random.random()
    assert p.mode == "boxes" and len(p.table) == 2
    assert np.array_equal(p.boxes_after[1], p.boxes_before[1])
    assert not np.array_equal(p.boxes_after[0], p.boxes_before[0]) and not np.array_equal(p.boxes_after[2], p.boxes_before[2])
    np.random.seed(seed)
    np.random.randint(0, 10)
    for _ in range(1 + A.MAX_ATTEMPTS + 1):
        np.random.uniform(-np.pi / 10, np.pi / 10)
        np.random.normal(), np.random.normal(), np.random.normal()
    assert np.random.random() == tail
    # the table's second entry is box 2's, and the moved labels keep box 1's line where it was
    from voxelnet_amd.targets import gt_standup_boxes
    assert np.array_equal(p.table[1]["lo"][:2], gt_standup_boxes(p.boxes_before[2:3])[0][:2])


def test_touching_footprints_do_not_collide_and_thin_overlaps_do():
    """the exact rule: shared edges / corners have no area; an overlap thinner than any raster cell is a collision"""
    from voxelnet_amd import augment as A
    a = np.array([0.0, 0.0, 0.0, 1.5, 2.0, 4.0, 0.0])
    for fn in (A.footprints_overlap, R.overlap):
        assert not fn(a, np.array([4.0, 0.0, 0.0, 1.5, 2.0, 4.0, 0.0]))               # shared edge x = 2
        assert fn(a, np.array([4.0 - 1e-9, 0.0, 0.0, 1.5, 2.0, 4.0, 0.0]))            # 1 nm of overlap
        assert not fn(a, np.array([4.0, 2.0, 0.0, 1.5, 2.0, 4.0, 0.0]))               # shared corner
        # a turned box on the diagonal: at (3, 3) only its OWN long axis separates the two (3 sqrt 2 = 4.243 >= 2 + 1.5 sqrt 2
        # = 4.121; on x, y and its short axis the projections overlap), at (2.9, 2.9) nothing does
        assert not fn(a, np.array([3.0, 3.0, 0.0, 1.5, 2.0, 4.0, np.pi / 4]))
        assert fn(a, np.array([2.9, 2.9, 0.0, 1.5, 2.0, 4.0, np.pi / 4]))
        assert fn(a, a)


def test_augment_labels_round_trip_within_the_two_decimal_format():
    """augment_labels -> label_to_gt_box_3d gives the moved boxes back within what two decimals can hold: each printed
    field is off by at most 0.005, so h / w / l by 0.005; the camera-frame centre by a vector of norm <= 0.005 sqrt(3),
    which the inverse calibration (T_velo_to_cam^-1 R_rect^-1, linear part) stretches by at most its spectral norm; the
    angle by 0.005 modulo pi, except that _limit_angle snaps anything within 5 degrees above -pi/2 to +pi/2 (the same
    line modulo pi: the circular distance stays within 5 degrees + 0.005 there)"""
    from voxelnet_amd import augment as A
    from voxelnet_amd import targets as T
    half = 0.005
    lin = np.matmul(T._T_VELO_2_CAM_INV, T._R_RECT_0_INV)[:3, :3]
    pos_bound = np.linalg.norm(lin, 2) * half * np.sqrt(3) + 1e-9
    snap = 5 / 180 * np.pi
    checked = set()
    for seed in range(60):
        labels = _labels(seed, 6)
        np.random.seed(seed)
        p = A.draw_augmentation(labels)
        lines = A.augment_labels(labels, p)
        assert len(lines) == len(labels) and [l.split()[0] for l in lines] == [l.split()[0] for l in labels]
        back = T.label_to_gt_box_3d([lines], "", "lidar")[0]
        assert back.shape == p.boxes_after.shape
        # the DontCare line (about 1 km away, |coordinates| ~ 1000) included: the bound does not depend on the position
        assert np.abs(back[:, :3] - p.boxes_after[:, :3]).max() <= pos_bound, seed
        assert np.abs(back[:, 3:6] - p.boxes_after[:, 3:6]).max() <= half + 1e-9, seed
        for r0, r1 in zip(p.boxes_after[:, 6], back[:, 6]):
            d = abs((r1 - r0 + np.pi / 2) % np.pi - np.pi / 2)                # circular distance modulo pi
            in_snap_zone = abs((r0 + np.pi / 2) % np.pi) < snap + half or abs((r0 + np.pi / 2) % np.pi - np.pi) < half
            assert d <= half + 1e-9 or (in_snap_zone and d <= snap + half + 1e-9), (seed, r0, r1)
        # and the Car-only boxes the target generator will read are the Car rows of the same set
        cars = T.label_to_gt_box_3d([lines], "Car", "lidar")[0]
        assert cars.shape[0] == sum(l.split()[0] in ("Car", "Van") for l in labels)
        checked.add(p.mode)
    assert checked == {"boxes", "rotate", "scale"}
    with pytest.raises(ValueError):
        A.augment_labels(labels[:-1], p)


def test_vn_augment_points_argument_checks():
    """null pointers -> VN_EINVAL; n == 0 -> 0 whatever the pointers; bad mode / table size -> VN_EINVAL; a misaligned
    cloud -> VN_EUNSUPPORTED.  No kernel is launched by any of these calls."""
    from voxelnet_amd import _lib
    lib = _lib.load()
    f = lib.vn_augment_points
    assert f(None, 10, _lib.VN_AUGMENT_ROTATE, None, 0, 1.0, 0.0, 1.0, None, None) == -1
    assert f(None, 10, _lib.VN_AUGMENT_SCALE, None, 0, 1.0, 0.0, 1.0, None, None) == -1
    assert f(None, 10, _lib.VN_AUGMENT_BOXES, None, 0, 1.0, 0.0, 1.0, None, None) == -1
    for mode in (_lib.VN_AUGMENT_BOXES, _lib.VN_AUGMENT_ROTATE, _lib.VN_AUGMENT_SCALE):
        assert f(None, 0, mode, None, 0, 1.0, 0.0, 1.0, None, None) == 0
    assert f(None, -1, _lib.VN_AUGMENT_SCALE, None, 0, 1.0, 0.0, 1.0, None, None) == -1
    assert f(None, 0, 3, None, 0, 1.0, 0.0, 1.0, None, None) == -1
    assert f(None, 0, -1, None, 0, 1.0, 0.0, 1.0, None, None) == -1
    assert f(None, 0, _lib.VN_AUGMENT_BOXES, None, _lib.VN_AUGMENT_MAX_BOXES + 1, 1.0, 0.0, 1.0, None, None) == -1
    assert f(None, 0, _lib.VN_AUGMENT_BOXES, None, -1, 1.0, 0.0, 1.0, None, None) == -1
    # non-null but never dereferenced on the host: a table is required when n_boxes > 0, 16-byte alignment of the cloud
    assert f(ctypes.c_void_p(4096), 10, _lib.VN_AUGMENT_BOXES, None, 2, 1.0, 0.0, 1.0, ctypes.c_void_p(4096), None) == -1
    assert f(ctypes.c_void_p(4100), 10, _lib.VN_AUGMENT_SCALE, None, 0, 1.0, 0.0, 1.0, ctypes.c_void_p(4096), None) == -2
    assert f(ctypes.c_void_p(4096), 10, _lib.VN_AUGMENT_BOXES, None, 0, 1.0, 0.0, 1.0, ctypes.c_void_p(4096), None) == 0   # in place, no box
    assert _lib.ABI_VERSION == lib.vn_abi_version() == 4                  # the symbol is additive


def test_box_table_entry_matches_the_header_layout(tmp_path):
    """vnAugmentBox: the C header, the ctypes structure and the NumPy record the table is staged from agree on size and
    on every field offset (64 bytes: six float32 bounds, five float64 values)"""
    import os
    from voxelnet_amd import _lib
    from voxelnet_amd import augment as A
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "layout.c"
    names = ["lo", "hi", "tx", "ty", "tz", "c", "s"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "voxelnet_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vnAugmentBox));\n'
                   + "".join(f'  printf(" %zu", offsetof(vnAugmentBox, {n}));\n' for n in names)
                   + '  printf(" %d %d\\n", VN_AUGMENT_MAX_BOXES, VN_AUGMENT_BOXES + 10 * VN_AUGMENT_ROTATE + 100 * VN_AUGMENT_SCALE);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    st = _lib.VnAugmentBox
    assert got[:8] == [ctypes.sizeof(st)] + [getattr(st, n).offset for n in names] == [64, 0, 12, 24, 32, 40, 48, 56]
    dt = A.BOX_DTYPE
    assert dt.itemsize == 64 and [dt.fields[n][1] for n in ("lo", "hi", "t", "c", "s")] == [0, 12, 24, 48, 56]
    assert got[8] == _lib.VN_AUGMENT_MAX_BOXES == A.MAX_BOXES == 128
    assert got[9] == _lib.VN_AUGMENT_BOXES + 10 * _lib.VN_AUGMENT_ROTATE + 100 * _lib.VN_AUGMENT_SCALE


def test_points_have_no_cpu_path():
    import torch
    from voxelnet_amd import _lib
    from voxelnet_amd import augment as A
    np.random.seed(0)
    p = A.draw_augmentation(_labels())
    with pytest.raises(_lib.VoxelnetHipError):
        A.augment_points_device(torch.zeros(8, 4), p)
    with pytest.raises(_lib.VoxelnetHipError):
        A.augment_points_device(np.zeros((8, 4), np.float32), p)


def test_dataset_still_refuses_and_names_the_switch(tmp_path):
    from voxelnet_amd import dataset as D
    with pytest.raises(NotImplementedError, match="DeviceBatcher"):
        D.KITTIDataset(str(tmp_path), augment=True)


def test_synthetic_frames_hold_points_inside_the_cars(tmp_path):
    """the frames tests/test_gpu_augment.py moves on the device, checked here with the restatement alone: each holds
    tens of points inside the six cars' bounds (so box perturbation cannot pass vacuously) and none in the DontCare box"""
    from voxelnet_amd import synth
    for f in range(4):
        cloud = synth.synth_cloud("Car", 6000, synth.frame_seed(2, f), 2.3, 35)
        labels = synth.synth_labels("Car", 6, f)
        boxes = R.label_to_gt_box_3d([labels], "", "lidar")[0]
        inside = []
        for b in boxes:
            lo, hi = R.bounds(b)
            inside.append(int(((cloud[:, :3] >= lo) & (cloud[:, :3] <= hi)).all(1).sum()))
        assert 69 <= sum(inside[:6]) <= 191 and inside[6] == 0, (f, inside)
        assert np.abs(boxes[6, :3]).max() > 900
