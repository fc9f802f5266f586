"""CPU: the host half of the part-aware object augmentation (voxelnet_amd/part_augment.py: PartRecipe, draw_parts, the
table check) — the order in which the draw consumes np.random, the pairing rules — the restatement's closed forms
(tests/part_augment_ref.py: hand-picked points whose owner and pyramid are written down), the swap geometry, and the
argument checks and struct layout of `vn_part_augment`.  The per-point work has no CPU path: tests/test_gpu_part_augment.py
checks it on the device against the restatement."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import part_augment_ref as R


def _line(cls, x, y, z, h, w, l, r):
    from voxelnet_amd.targets import lidar_box_to_label_line
    return lidar_box_to_label_line(cls, [x, y, z, h, w, l, r])


DONTCARE = "DontCare -1 -1 -10 0 0 0 0 -1 -1 -1 -1000 -1000 -1000 -10"


def _mixed(n_car=5, n_ped=3, n_cyc=1):
    """cars, pedestrians and one cyclist interleaved, a DontCare line in the middle"""
    lines = []
    for i in range(max(n_car, n_ped, n_cyc)):
        if i < n_car:
            lines.append(_line("Car", 10.0 + 6 * i, -3.0, -1.7, 1.5 + 0.05 * i, 1.6, 3.9 + 0.1 * i, 0.1 * i))
        if i == 1:
            lines.append(DONTCARE)
        if i < n_ped:
            lines.append(_line("Pedestrian", 10.0 + 4 * i, 6.0, -1.6, 1.7 + 0.03 * i, 0.6, 0.8, 0.3))
        if i < n_cyc:
            lines.append(_line("Cyclist", 20.0, 12.0, -1.6, 1.7, 0.6, 1.8, -0.4))
    return lines


# ---------------------------------------------------------------------------------------------------------------------
# closed forms of the restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_hand_picked_points_have_the_owner_and_pyramid_written_down():
    cloud, boxes, want_owner, want_face = R.edge_points()
    table = [R.entry(b) for b in boxes]
    own, face = R.owner_face(cloud, table)
    assert own.tolist() == want_owner.tolist()
    assert face.tolist() == want_face.tolist()
    # every pyramid of both boxes, every kind of row
    assert {(o, f) for o, f in zip(want_owner, want_face) if o >= 0} == {(o, f) for o in (0, 1) for f in range(6)}
    assert (want_owner == -1).sum() >= 15 and np.isnan(cloud[:, :3]).any(1).sum() == 3
    out, counts, stats = R.apply(cloud, table)
    assert out.tobytes() == cloud.tobytes() and not stats.any()          # nothing marked: a bit copy, NaN payloads included
    assert counts.tolist() == [np.bincount(want_face[want_owner == o], minlength=6).tolist() for o in (0, 1)]
    # the same points, every pyramid of box A dropped: exactly A's rows become NaN points
    out, counts2, stats = R.apply(cloud, [R.entry(boxes[0], drop=0x3F), R.entry(boxes[1])])
    assert np.array_equal(counts2, counts) and stats.tolist() == [[int((want_owner == 0).sum()), 0, 0], [0, 0, 0]]
    assert (out.view(np.uint32)[want_owner == 0] == 0x7FC00000).all()
    assert out[want_owner != 0].tobytes() == cloud[want_owner != 0].tobytes()


def test_fmix32_is_the_murmur3_finalizer():
    """published values of MurmurHash3's fmix32, and the wrap-around"""
    assert [int(v) for v in R.fmix32(np.array([0, 1, 2, 0xFFFFFFFF], dtype=np.uint64))] == [0, 0x514E28B7, 0x30F4C306, 0x81F16F39]
    import shuffle_ref as S
    xs = np.random.default_rng(0).integers(0, 2 ** 32, 1000, dtype=np.uint64)
    assert np.array_equal(R.fmix32(xs), S.fmix32(xs))                    # the shuffle's restatement of the same function


def test_swap_maps_corners_to_the_partners_corners():
    """the eight corners of a box, through the local coordinates and the swap, land on the partner's corners to 1e-12
    (float64, before the rounding); the ratios are draw_parts' own"""
    from voxelnet_amd import part_augment as P
    labels = [_line("Car", 12.0, -3.0, -1.7, 1.5, 1.6, 3.9, 0.4), _line("Car", 31.0, 8.0, -1.2, 1.9, 2.1, 5.2, -2.3)]
    np.random.seed(0)
    p = P.draw_parts(labels, P.PartRecipe(drop_prob=None, sparse_prob=None, swap_prob=1.0))
    t = R.from_params(p)
    assert [e["swap_with"] for e in t] == [1, 0] and t[0]["swap_mask"] == t[1]["swap_mask"] != 0
    for a, b in ((0, 1), (1, 0)):
        ea, eb = t[a], t[b]
        for su in (-1, 1):
            for sv in (-1, 1):
                for sw in (-1, 1):
                    def corner(e):
                        cu, cv, hh = su * e["hl"], sv * e["hw"], (e["z1"] - e["z0"]) / 2
                        return np.array([e["x"] + cu * e["c"] - cv * e["s"], e["y"] + cu * e["s"] + cv * e["c"], e["z0"] + hh + sw * hh])
                    ca = corner(ea)
                    u, v, w = R.local(ca[0], ca[1], ca[2], ea)
                    got = np.array(R.swap_xyz(u, v, w, ea, eb))
                    assert np.abs(got - corner(eb)).max() <= 1e-12, (a, su, sv, sw)


def test_thinning_keeps_the_stated_share():
    """a pyramid of 4,000 rows thinned with keep = 0.5, 0.25, 1, 0: the kept share is within 4 standard deviations"""
    rng = np.random.default_rng(5)
    box = np.array([20.0, 0.0, -1.0, 2.0, 2.0, 4.0, 0.3])
    q = rng.uniform(0.05, 0.95, 4000)[:, None] * np.array([2.0, 0.0, 0.0])          # on the +u axis: pyramid 0
    c, s = np.cos(box[6]), np.sin(box[6])
    cloud = np.stack([box[0] + q[:, 0] * c, box[1] + q[:, 0] * s, np.zeros(4000), np.ones(4000)], 1).astype(np.float32)
    for keep in (0.5, 0.25, 1.0, 0.0):
        t = [R.entry(box, sparse=1, key=0xDEADBEEF, thresh=int(np.floor(keep * 2 ** 24)), min_points=16)]
        out, counts, stats = R.apply(cloud, t)
        assert counts[0].tolist() == [4000, 0, 0, 0, 0, 0]
        kept = 4000 - int(stats[0][1])
        assert int(np.isnan(out[:, 0]).sum()) == stats[0][1] and stats[0][0] == stats[0][2] == 0
        assert abs(kept - 4000 * keep) <= 4 * np.sqrt(4000 * keep * (1 - keep)) + 1e-9, (keep, kept)


# ---------------------------------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------------------------------
def test_an_all_off_recipe_draws_nothing():
    from voxelnet_amd import part_augment as P
    labels = _mixed()
    for off in (dict(drop_prob=None, sparse_prob=None, swap_prob=None), dict(drop_prob=0, sparse_prob=0.0, swap_prob=0)):
        np.random.seed(4)
        state = np.random.get_state()
        p = P.draw_parts(labels, P.PartRecipe(**off))
        after = np.random.get_state()
        assert state[0] == after[0] and np.array_equal(state[1], after[1]) and state[2:] == after[2:]
        assert len(p.table) == 9 and p.entry_line == [i for i, line in enumerate(labels) if not line.startswith("DontCare")]
        assert not p.table["drop_mask"].any() and not p.table["sparse_mask"].any() and not p.table["swap_mask"].any()
        assert (p.table["swap_with"] == -1).all() and (p.table["ru"] == 1).all()
    # the boxes are gtsample.box_table's
    from voxelnet_amd import gtsample as G
    from voxelnet_amd.targets import label_to_gt_box_3d
    boxes = label_to_gt_box_3d([labels], "", "lidar")[0][p.entry_line]
    assert np.array_equal(p.boxes, boxes)
    base = G.box_table(boxes)
    assert all(np.array_equal(p.table[n], base[n]) for n in base.dtype.names)


def test_each_stage_consumes_exactly_the_documented_draws():
    from voxelnet_amd import part_augment as P
    from voxelnet_amd.targets import label_to_gt_box_3d
    labels = _mixed()
    lines = [i for i, line in enumerate(labels) if not line.startswith("DontCare")]
    boxes = label_to_gt_box_3d([labels], "", "lidar")[0][lines]
    g = len(lines)
    off = dict(drop_prob=None, sparse_prob=None, swap_prob=None)
    hits = 0
    for seed in range(20):
        # drop alone
        np.random.seed(seed)
        p = P.draw_parts(labels, P.PartRecipe(**{**off, "drop_prob": 0.4}))
        tail = np.random.random()
        np.random.seed(seed)
        want = [(1 << int(np.random.randint(0, 6))) if np.random.random() < 0.4 else 0 for _ in range(g)]
        assert np.random.random() == tail and p.table["drop_mask"].tolist() == want
        assert not p.table["sparse_mask"].any() and not p.table["swap_mask"].any()
        # thin alone
        np.random.seed(seed)
        p = P.draw_parts(labels, P.PartRecipe(**{**off, "sparse_prob": 0.4, "sparse_keep": 0.3, "sparse_min": 7}))
        tail = np.random.random()
        np.random.seed(seed)
        want = []
        for _ in range(g):
            if np.random.random() < 0.4:
                f = int(np.random.randint(0, 6))
                want.append((1 << f, int(np.random.randint(0, 2 ** 32, dtype=np.uint32)), int(np.floor(0.3 * 2 ** 24)), 7))
            else:
                want.append((0, 0, 0, 0))
        assert np.random.random() == tail
        assert [(int(r["sparse_mask"]), int(r["sparse_key"]), int(r["sparse_thresh"]), int(r["sparse_min"])) for r in p.table] == want
        # swap alone
        np.random.seed(seed)
        p = P.draw_parts(labels, P.PartRecipe(**{**off, "swap_prob": 0.6}))
        tail = np.random.random()
        np.random.seed(seed)
        types = {}
        for k, i in enumerate(lines):
            types.setdefault(labels[i].split()[0], []).append(k)
        assert list(types) == ["Car", "Pedestrian", "Cyclist"]                 # order of first appearance
        want_with, want_mask = [-1] * g, [0] * g
        for members in types.values():
            if len(members) < 2:
                continue                                                     # the lone cyclist: no permutation drawn
            order = [members[j] for j in np.random.permutation(len(members))]
            for a, b in zip(order[0::2], order[1::2]):
                if np.random.random() < 0.6:
                    f = int(np.random.randint(0, 6))
                    want_with[a], want_with[b], want_mask[a], want_mask[b] = b, a, 1 << f, 1 << f
                    hits += 1
        assert np.random.random() == tail
        assert p.table["swap_with"].tolist() == want_with and p.table["swap_mask"].tolist() == want_mask
        for k in range(g):
            o = want_with[k]
            want_r = (1.0, 1.0, 1.0) if o < 0 else tuple((boxes[o, j] / 2) / (boxes[k, j] / 2) for j in (5, 4, 3))
            assert (p.table[k]["ru"], p.table[k]["rv"], p.table[k]["rw"]) == want_r
    assert hits >= 20
    # all three: drop for every entry, then thin for every entry, then the swaps
    np.random.seed(99)
    p = P.draw_parts(labels, P.PartRecipe(drop_prob=0.5, sparse_prob=0.5, swap_prob=0.5))
    tail = np.random.random()
    np.random.seed(99)
    d = P.draw_parts(labels, P.PartRecipe(drop_prob=0.5, sparse_prob=None, swap_prob=None))
    s = P.draw_parts(labels, P.PartRecipe(drop_prob=None, sparse_prob=0.5, swap_prob=None))
    w = P.draw_parts(labels, P.PartRecipe(drop_prob=None, sparse_prob=None, swap_prob=0.5))
    assert np.random.random() == tail
    assert np.array_equal(p.table["drop_mask"], d.table["drop_mask"]) and np.array_equal(p.table["sparse_key"], s.table["sparse_key"])
    assert np.array_equal(p.table["sparse_mask"], s.table["sparse_mask"]) and np.array_equal(p.table["swap_with"], w.table["swap_with"])
    assert np.array_equal(p.table["swap_mask"], w.table["swap_mask"]) and np.array_equal(p.table["ru"], w.table["ru"])


def test_swaps_stay_inside_a_type_and_an_entry_swaps_at_most_once():
    from voxelnet_amd import part_augment as P
    labels = _mixed(7, 4, 2)
    swaps = 0
    for seed in range(50):
        np.random.seed(seed)
        p = P.draw_parts(labels, P.PartRecipe(swap_prob=0.9))
        kinds = [labels[i].split()[0] for i in p.entry_line]
        for k, row in enumerate(p.table):
            o = int(row["swap_with"])
            if o < 0:
                assert row["swap_mask"] == 0
                continue
            swaps += 1
            assert o != k and kinds[o] == kinds[k]
            assert int(p.table[o]["swap_with"]) == k and p.table[o]["swap_mask"] == row["swap_mask"]          # mutual: one partner each
            assert bin(int(row["swap_mask"])).count("1") == 1 and row["swap_mask"] < 64
            assert row["ru"] * p.table[o]["ru"] == pytest.approx(1.0, abs=1e-15)
        for name in ("drop_mask", "sparse_mask"):
            assert all(bin(int(m)).count("1") <= 1 and m < 64 for m in p.table[name])
    assert swaps >= 200


def test_a_pair_with_a_non_positive_extent_draws_the_same_numbers_and_gets_no_swap():
    from voxelnet_amd import part_augment as P
    good = [_line("Car", 10.0, 0.0, -1.7, 1.5, 1.6, 3.9, 0.1), _line("Car", 20.0, 0.0, -1.7, 1.5, 1.6, 3.9, 0.1)]
    flat = [good[0], _line("Car", 20.0, 0.0, -1.7, 0.0, 1.6, 3.9, 0.1)]          # h = 0
    tails = []
    for labels in (good, flat):
        np.random.seed(3)
        p = P.draw_parts(labels, P.PartRecipe(drop_prob=None, sparse_prob=None, swap_prob=1.0))
        tails.append(np.random.random())
        assert (p.table["swap_with"].tolist() == [1, 0]) == (labels is good)
        if labels is flat:
            assert not p.table["swap_mask"].any() and (p.table["ru"] == 1).all() and (p.table["rw"] == 1).all()
    assert tails[0] == tails[1]


def test_129_boxes_raise_and_128_do_not():
    from voxelnet_amd import _lib
    from voxelnet_amd import part_augment as P
    labels = [_line("Car", 10.0 * (i % 13), 10.0 * (i // 13) - 50, -1.7, 1.5, 1.6, 3.9, 0.1) for i in range(P.MAX_BOXES + 1)]
    with pytest.raises(_lib.VoxelnetHipError):
        P.draw_parts(labels, P.PartRecipe())
    assert len(P.draw_parts(labels[:-1] + [DONTCARE], P.PartRecipe()).table) == P.MAX_BOXES == 128


def test_the_recipe_is_validated():
    from voxelnet_amd import part_augment as P
    r = P.PartRecipe()
    assert (r.drop_prob, r.sparse_prob, r.sparse_keep, r.sparse_min, r.swap_prob) == (0.25, 0.25, 0.5, 16, 0.25)
    for bad in (dict(drop_prob=-0.1), dict(drop_prob=1.5), dict(sparse_prob="0.5"), dict(swap_prob=float("nan")), dict(swap_prob=True),
                dict(sparse_keep=None), dict(sparse_keep=1.01), dict(sparse_min=-1), dict(sparse_min=2.5), dict(sparse_min=2 ** 31)):
        with pytest.raises(ValueError):
            P.PartRecipe(**bad)
    P.PartRecipe(drop_prob=None, sparse_prob=0, swap_prob=1, sparse_keep=0, sparse_min=0)


# ---------------------------------------------------------------------------------------------------------------------
# the C side and the wrapper
# ---------------------------------------------------------------------------------------------------------------------
def test_vn_part_augment_argument_checks():
    """the stated status codes; every check runs before any launch, so none of these calls needs a GPU"""
    from voxelnet_amd import _lib
    lib = _lib.load()
    f, wsb = lib.vn_part_augment, lib.vn_part_augment_workspace_bytes
    ok, ok2, ws, bad = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 21), ctypes.c_void_p(4100)
    odd = ctypes.c_void_p(4098)
    big = 1 << 20
    assert wsb(1000, 8) >= 2000 and wsb(1000, 8) % 16 == 0 and wsb(0, 8) == 0 and wsb(1000, 0) == 0
    assert wsb(-1, 8) == 0 and wsb(1 << 31, 8) == 0 and wsb(10, -1) == 0 and wsb(10, 129) == 0          # bad arguments
    assert wsb((1 << 31) - 1, 128) >= 2 * ((1 << 31) - 1)
    # (points, n, boxes, n_boxes, gate, gate_first, gate_min, out, counts, stats, workspace, workspace_bytes, stream)
    assert f(None, 0, None, 0, None, 0, 0, None, None, None, None, 0, None) == 0                         # nothing at all
    assert f(ok, 10, None, 0, None, 0, 0, ok, None, None, None, 0, None) == 0                            # in place, no entries: nothing
    assert f(None, -1, None, 0, None, 0, 0, None, None, None, None, 0, None) == -1
    assert f(ok, 1 << 31, None, 0, None, 0, 0, ok, None, None, None, 0, None) == -1
    assert f(ok, 10, ok2, -1, None, 0, 0, ok, ok2, ok2, ws, big, None) == -1
    assert f(ok, 10, ok2, 129, None, 0, 0, ok, ok2, ok2, ws, big, None) == -1
    assert f(ok, 10, ok2, 4, None, -1, 0, ok, ok2, ok2, ws, big, None) == -1                             # gate_first outside [0, n_boxes]
    assert f(ok, 10, ok2, 4, ok2, 5, 0, ok, ok2, ok2, ws, big, None) == -1
    assert f(None, 10, ok2, 4, None, 0, 0, ok, ok2, ok2, ws, big, None) == -1                            # null pointers with work to do
    assert f(ok, 10, ok2, 4, None, 0, 0, None, ok2, ok2, ws, big, None) == -1
    assert f(ok, 10, None, 4, None, 0, 0, ok, ok2, ok2, ws, big, None) == -1
    assert f(ok, 10, ok2, 4, None, 0, 0, ok, None, ok2, ws, big, None) == -1
    assert f(ok, 10, ok2, 4, None, 0, 0, ok, ok2, None, ws, big, None) == -1
    assert f(ok, 10, ok2, 4, None, 0, 0, ok, ok2, ok2, None, big, None) == -1
    assert f(ok, 10, ok2, 4, None, 0, 0, ctypes.c_void_p(4096 + 32), ok2, ok2, ws, big, None) == -1      # out overlaps points
    assert f(ctypes.c_void_p(4096 + 144), 10, ok2, 4, None, 0, 0, ok, ok2, ok2, ws, big, None) == -1
    assert f(ok, 10, ok2, 4, None, 0, 0, ok, ok2, ok2, ws, wsb(10, 4) - 1, None) == -3                   # workspace too small
    assert f(ok, 1000, ok2, 4, None, 0, 0, ok, ok2, ok2, ws, wsb(999, 4) - 16, None) == -3
    assert f(bad, 10, ok2, 4, None, 0, 0, ok2, ok2, ok2, ws, big, None) == -2                            # off the 16-byte alignment
    assert f(ok, 10, ok2, 4, None, 0, 0, ctypes.c_void_p((1 << 22) + 4), ok2, ok2, ws, big, None) == -2
    assert f(ok, 10, ctypes.c_void_p((1 << 20) + 8), 4, None, 0, 0, ok, ok2, ok2, ws, big, None) == -2
    assert f(ok, 10, ok2, 4, None, 0, 0, ok, ok2, ok2, ctypes.c_void_p((1 << 21) + 8), big, None) == -2
    assert f(ok, 10, ok2, 4, None, 0, 0, ok, odd, ok2, ws, big, None) == -2                              # off the 4-byte alignment
    assert f(ok, 10, ok2, 4, None, 0, 0, ok, ok2, odd, ws, big, None) == -2
    assert f(ok, 10, ok2, 4, odd, 0, 0, ok, ok2, ok2, ws, big, None) == -2
    assert _lib.ABI_VERSION == lib.vn_abi_version() == 4                                                 # the symbols are additive
    assert {"vn_part_augment", "vn_part_augment_workspace_bytes"} <= set(_lib.SIGNATURES) and _lib.VN_PART_MAX_BOXES == 128


def test_the_struct_matches_the_header_layout(tmp_path):
    """vnPartBox: the C header, the ctypes structure and the NumPy record the table is staged from agree on the size and on
    every field offset; it begins with vnGtBox's eight fields"""
    from voxelnet_amd import _lib
    from voxelnet_amd import gtsample as G
    from voxelnet_amd import part_augment as P
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = ["x", "y", "z0", "z1", "hl", "hw", "c", "s", "ru", "rv", "rw", "drop_mask", "sparse_mask", "swap_mask", "swap_with",
             "sparse_key", "sparse_thresh", "sparse_min", "reserved", "pad"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "voxelnet_hip.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(vnPartBox));\n'
                   + "".join(f'  printf(" %zu", offsetof(vnPartBox, {n}));\n' for n in names)
                   + '  printf("\\n%d\\n", VN_PART_MAX_BOXES);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    got = [int(v) for v in out[0].split()]
    assert got == [128] + [8 * i for i in range(11)] + [88 + 4 * i for i in range(8)] + [120]
    assert got == [ctypes.sizeof(_lib.VnPartBox)] + [getattr(_lib.VnPartBox, n).offset for n in names]
    assert got == [P.PART_DTYPE.itemsize] + [P.PART_DTYPE.fields[n][1] for n in names]
    assert [G.BOX_DTYPE.fields[n][1] for n in names[:8]] == got[1:9]
    assert int(out[1]) == _lib.VN_PART_MAX_BOXES == P.MAX_BOXES


def test_the_wrapper_checks_the_table_on_the_host():
    import torch
    from voxelnet_amd import _lib
    from voxelnet_amd import part_augment as P
    boxes = np.array([[10.0, 0, -1, 2, 2, 4, 0.1], [20.0, 0, -1, 2, 2, 4, 0.2], [30.0, 0, -1, 2, 2, 4, 0.3]])
    for field, value in (("swap_with", 3), ("swap_with", -2), ("swap_with", 1 << 20), ("sparse_thresh", (1 << 24) + 1), ("sparse_min", -1)):
        t = P.part_table(boxes)
        t[1][field] = value
        with pytest.raises(ValueError, match=field):
            P.check_table(t)
        with pytest.raises(ValueError, match=field):          # the table is checked before the tensor is looked at
            P.enqueue_part_points(torch.zeros(8, 4), P.PartParams(t, [], boxes))
    t = P.part_table(boxes)
    t[1]["swap_with"], t[1]["sparse_thresh"], t[2]["swap_with"] = 2, 1 << 24, -1
    assert P.check_table(t).tobytes() == t.tobytes()
    with pytest.raises(_lib.VoxelnetHipError):
        P.check_table(P.part_table(np.tile(boxes[:1], (129, 1))))
    # no CPU path
    p = P.PartParams(P.part_table(boxes), [], boxes)
    for bad in (torch.zeros(8, 4), np.zeros((8, 4), np.float32)):
        with pytest.raises(_lib.VoxelnetHipError):
            P.part_points_device(bad, p)
        with pytest.raises(_lib.VoxelnetHipError):
            P.enqueue_part_points(bad, p)


def test_unknown_part_augment_values_raise(monkeypatch):
    """`part_augment` is None or a PartRecipe instance; the check comes before anything touches the device"""
    from voxelnet_amd import dataset as D
    from voxelnet_amd import part_augment as P
    monkeypatch.setattr(D, "pipeline_stream", lambda device: None)
    for bad in (True, False, 1, "parts", P.PartRecipe, {"drop_prob": 0.5}):
        with pytest.raises(ValueError, match="part_augment"):
            D.DeviceCollate("cuda:0", "Car", part_augment=bad)
        with pytest.raises(ValueError, match="part_augment"):
            D.DeviceBatcher([], "cuda:0", "Car", part_augment=bad)
    rec = P.PartRecipe()
    assert D.DeviceCollate("cuda:0", "Car", part_augment=rec).part_augment is rec
    assert D.DeviceCollate("cuda:0", "Car").part_augment is None
    assert D.DeviceBatcher([], "cuda:0", "Car", part_augment=rec).collate.part_augment is rec


def test_dense_cases_fill_every_pyramid_and_the_table_fires_every_branch():
    """the inputs tests/test_gpu_part_augment.py runs on the device, judged on the restatement alone: 5,921 rows, every
    pyramid of every box holds at least 21 points, a thinned pyramid keeps 28-76 %, and the hand-made table takes every
    branch of the rules"""
    for seed in (0, 1, 2):
        cloud, boxes = R.dense_case(seed)
        assert cloud.shape == (5921, 4) and cloud.dtype == np.float32 and len(cloud) % 256 != 0
        t = R.dense_table(boxes)
        own, face = R.owner_face(cloud, t)
        out, counts, stats = R.apply(cloud, t)
        assert (counts.sum(1) == 240).all() and counts.min() >= 21 and (own >= 0).sum() == 1920
        assert stats[0][0] == counts[0][0] and stats[0][1] == 0                       # dropped; drop beats thin on pyramid 0
        assert stats[0][2] == counts[0][2] and stats[1][2] == counts[1][2]            # the first swap pair
        assert 0.28 * counts[1][3] <= counts[1][3] - stats[1][1] <= 0.76 * counts[1][3] and stats[1][1] > 0          # thinned
        assert stats[2].tolist() == [0, 0, 0] and counts[2][1] < 64                   # NOT thinned: below its minimum
        assert stats[3].tolist() == [0, 0, int(counts[3][4])]                         # the second pair: 3 -> 5 moves
        assert stats[5].tolist() == [int(counts[5][4]), 0, 0]                         # ... 5 -> 3 is dropped first
        assert stats[4].tolist() == stats[6].tolist() == stats[7].tolist() == [0, 0, 0]          # no partner / itself / nothing
        changed = (out.view(np.uint32) != cloud.view(np.uint32)).any(1)
        assert changed.sum() == stats.sum() and not changed[own < 0].any()
        # swapped rows land inside the partner's box (to rounding) and in the same pyramid of it
        moved = (own == 0) & (face == 2)
        back_own, back_face = R.owner_face(out[moved], [R.entry(boxes[1])])
        assert (back_face[back_own == 0] == 2).all() and (back_own == 0).mean() > 0.9
