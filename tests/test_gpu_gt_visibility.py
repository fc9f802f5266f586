"""GPU: the occlusion-consistent paste — `vn_gt_paste_visible` (csrc/gtsample.hip through voxelnet_amd.gtsample) against
tests/visibility_ref.py, BIT-EQUAL: output rows (NaN rows in the same places), the count, the visible and kept counts
per object and the two statistics; and the `GTSampler(visibility=…)` switch of DeviceCollate / DeviceBatcher against a
host replay of the same shuffles and draws (voxel buffers = oracle voxelizer of the restatement's cloud, bit for bit;
labels without the rejected objects' lines)."""
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

import augment_ref as AR
import compose_ref as CR
import gtsample_ref as R
import visibility_ref as V
from oracle import voxelize as ov
from test_gt_visibility_host import SMALL, car_face, edge_points, hand_made_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PER_CLASS = {"Car": 15}
# a coarse grid for random clouds: many points per bin, so every rule fires on a few hundred points
COARSE = V.Grid(nu=64, nv=16, v_lo=-0.3, v_hi=0.1, margin=0.3, min_visible=2)


@functools.lru_cache(maxsize=None)
def _frame(f):
    from voxelnet_amd import synth
    cloud = synth.synth_cloud("Car", 6000, synth.frame_seed(2, f), 2.3, 35)
    cloud.setflags(write=False)
    return cloud, tuple(synth.synth_labels("Car", 6, f))


@functools.lru_cache(maxsize=None)
def _ref_db():
    """the restatement's database of frames 8..23: 96 objects, computed once and left unchanged"""
    return tuple(R.database([(f"{f:06d}", _frame(f)[0], list(_frame(f)[1])) for f in range(8, 24)]))


def _same(a, b):
    """bit-equal float32 arrays (NaN rows: NaN in the same places — a NaN's payload is not part of the contract)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def _visibility(grid):
    from voxelnet_amd import gtsample as G
    return G.Visibility(**dataclasses.asdict(grid))


def _params(boxes, obj, offsets):
    from voxelnet_amd import gtsample as G
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    return G.GTSampleParams(G.box_table(boxes), np.asarray(obj, dtype=np.float32).reshape(-1, 4), boxes, [],
                            np.asarray(offsets, dtype=np.int32))


def _dev(cloud, boxes, obj, offsets, grid, cap=None):
    """-> (out (cap,4), count, visible, kept, stats, accepted) of the device, all read back; the inputs are left alone"""
    from voxelnet_amd import gtsample as G
    cloud = np.array(cloud, dtype=np.float32).reshape(-1, 4)
    pts = torch.from_numpy(cloud.copy()).to(DEV)
    params = _params(boxes, obj, offsets)
    before = (params.points.copy(), params.table.copy(), params.offsets.copy())
    out, count, res = G.gt_paste_visible_device(pts, params, _visibility(grid), padded=True, cap=cap)
    got = (out.cpu().numpy(), int(count.item()), res.visible, res.kept, res.stats, res.accepted)
    assert np.array_equal(pts.cpu().numpy().view(np.uint32), cloud.view(np.uint32))
    assert params.points.tobytes() == before[0].tobytes() and params.table.tobytes() == before[1].tobytes()
    assert params.offsets.tobytes() == before[2].tobytes()
    return got


def _check(cloud, boxes, obj, offsets, grid, cap=None):
    """everything the call reports against the restatement -> the restatement's dict"""
    want = V.paste_visible(cloud, boxes, obj, offsets, grid, cap)
    out, count, visible, kept, stats, accepted = _dev(cloud, boxes, obj, offsets, grid, cap)
    assert visible.dtype == np.int32 and kept.dtype == np.int32 and stats.dtype == np.int32
    assert np.array_equal(visible, want["visible"]), (visible, want["visible"])
    assert np.array_equal(accepted, want["accepted"])
    assert np.array_equal(kept, want["kept"]), (kept, want["kept"])
    assert np.array_equal(stats, want["stats"]), (stats, want["stats"])
    assert count == want["count"], (count, want["count"])
    assert _same(out, want["out"]), int((out.view(np.uint32) != want["out"].view(np.uint32)).any(1).sum())
    assert np.isnan(out[count:]).all()
    return want


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", range(4))
def test_synthetic_frames_are_bit_equal_to_the_restatement(f):
    """objects [8f, 8f + 8) of the database's >= 5-point entries pasted into frame f, the default grid"""
    cloud, _ = _frame(f)
    big = [e for e in _ref_db() if len(e["points"]) >= 5]
    assert len(big) == 55
    es = big[8 * f:8 * f + 8]
    boxes = np.array([e["box"] for e in es])
    objs = [e["points"] for e in es]
    obj, off = np.concatenate(objs), V.offsets_of(objs)
    g = V.Grid()
    want = V.paste_visible(cloud, boxes, obj, off, g)
    sizes = np.diff(off)
    print(f"frame {f}: stats {want['stats'].tolist()}, visible {want['visible'].tolist()} of {sizes.tolist()}, kept {want['kept'].tolist()}")
    # on the restatement alone: every branch is taken
    assert (~want["accepted"]).sum() >= 1
    assert (want["accepted"] & (want["visible"] > 0) & (want["visible"] < sizes)).sum() >= 1
    assert want["stats"][1] >= 1 and want["stats"][0] >= 1
    _check(cloud, boxes, obj, off, g)
    a, b = _dev(cloud, boxes, obj, off, g), _dev(cloud, boxes, obj, off, g)          # two runs give the same bits
    assert a[1] == b[1] and _same(a[0], b[0]) and all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))


def _cubes(rng, g):
    return np.stack([rng.uniform(4, 38, g), rng.uniform(-18, 18, g), rng.uniform(-3, -0.5, g), np.full(g, 1.5), np.full(g, 1.5),
                     np.full(g, 1.5), rng.uniform(-np.pi / 2, np.pi / 2, g)], 1).reshape(g, 7)


def _cloud(rng, n, boxes=None):
    """n points all round the sensor, z / range mostly inside COARSE's rows; with boxes: a third of them near a box centre"""
    pts = np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(-3, 1, n), np.round(rng.uniform(0, 1, n), 2)], 1)
    if boxes is not None and len(boxes) and n:
        near = rng.random(n) < 0.33
        which = rng.integers(0, len(boxes), n)
        centre = boxes[which][:, :3] + np.array([0.0, 0.0, 0.75])
        pts[near, :3] = (centre + rng.uniform(-1.5, 1.5, (n, 3)))[near]
    return np.ascontiguousarray(pts, dtype=np.float32)


def _split(rng, m, g):
    """offsets of m rows over g objects, some of them empty"""
    if g == 0:
        return np.zeros(1, dtype=np.int32)
    cuts = np.sort(rng.integers(0, m + 1, g - 1)) if g > 1 else np.zeros(0, dtype=np.int64)
    return np.concatenate([[0], cuts, [m]]).astype(np.int32)


@pytest.mark.parametrize("n_boxes", [0, 1, 128])
def test_block_edges(n_boxes):
    from voxelnet_amd import _lib
    rng = np.random.default_rng(17 + n_boxes)
    boxes = _cubes(rng, n_boxes)
    seen = np.zeros(4, dtype=np.int64)
    for n in (0, 1, 255, 256, 257):
        for m in (0, 1, 300):
            cloud = _cloud(rng, n, boxes)
            obj = _cloud(rng, m)
            if n_boxes == 0 and m > 0:                   # rows without an object: offsets[n_boxes] != m
                with pytest.raises(_lib.VoxelnetHipError, match="invalid argument"):
                    _dev(cloud, boxes, obj, [0], COARSE)
                continue
            off = _split(rng, m, n_boxes)
            want = _check(cloud, boxes, obj, off, COARSE)
            seen += [want["stats"][0], want["stats"][1], (~want["accepted"]).sum(), want["visible"].sum() - want["kept"].sum()]
    if n_boxes:
        assert seen[1] > 0 and seen[2] > 0 and seen[3] > 0, seen          # shadows, rejections, culled object points
    if n_boxes == 128:
        assert seen[0] > 0, seen


def test_rows_on_both_sides_of_the_scans_carry():
    """the one-workgroup scan takes 256 counts per trip: its carry starts at concatenated row 65,536 — inside the
    object segment (n = 65,400, m = 300) and inside the scene (n = 65,537, m = 0)"""
    rng = np.random.default_rng(5)
    boxes = _cubes(rng, 128)
    cloud, obj = _cloud(rng, 65_400, boxes), _cloud(rng, 300)
    off = _split(rng, 300, 128)
    g = dataclasses.replace(COARSE, nu=512, nv=64, margin=1.0)
    want = _check(cloud, boxes, obj, off, g)
    keep = want["obj_keep"]
    assert keep[:136].any() and keep[136:].any() and not keep.all() and 0 < want["scene_keep"].sum() < 65_400
    cloud = _cloud(rng, 65_537, boxes)
    want = _check(cloud, boxes[:1], np.zeros((0, 4), np.float32), [0, 0], g)
    assert want["scene_keep"][65_536] and want["count"] == 65_537 and want["visible"].tolist() == [0]
    cloud[65_530] = np.nan
    want = _check(cloud, boxes[:1], np.zeros((0, 4), np.float32), [0, 0], g)
    assert want["count"] == 65_536


def _far_boxes(g):
    return np.array([[500.0 + 10 * i, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0] for i in range(g)])


def test_closed_form_edge_points():
    """the hand-picked points of the host test as the scene; as objects the same points (equal depth: visible at margin
    0) and their doubles (same u and v exactly, twice the depth: hidden wherever the point has a bin)"""
    table = edge_points()
    pts = np.array([list(p) + [0.5] for p, _, _ in table], dtype=np.float32)
    has_bin = np.array([b is not None for _, b, _ in table])
    front = {}                                          # the nearest hand-picked point of every bin, from the closed forms
    for _, b, d in table:
        if b is not None:
            front[b] = min(front.get(b, np.inf), d)
    first = np.array([b is None or d == front[b] for _, b, d in table])
    assert has_bin.sum() == 17 and (~first).sum() == 3         # some bins hold two of the points
    doubles = pts * np.float32([2, 2, 2, 1])
    obj = np.concatenate([pts, doubles])
    k = len(pts)
    off = np.arange(2 * k + 1, dtype=np.int32)          # one object per point
    g = dataclasses.replace(SMALL, min_visible=1)
    want = _check(pts, _far_boxes(2 * k), obj, off, g)
    nan = np.isnan(pts[:, :3]).any(1)
    assert want["visible"][:k].tolist() == (~nan & first).astype(int).tolist()
    assert want["visible"][k:].tolist() == (~nan & ~has_bin).astype(int).tolist()
    # equal depths shadow nobody: only the second point of a bin lies behind the first one's pasted copy
    assert want["scene_keep"].tolist() == (~nan & first).tolist() and want["stats"].tolist() == [0, int((~first).sum())]
    # and the other way round: the doubles as the scene, the points as objects
    want = _check(doubles, _far_boxes(k), pts, off[:k + 1], g)
    assert want["stats"][0] == 0 and want["stats"][1] >= 10


def test_equal_depths_go_to_the_lower_object_and_cull_nobody():
    g = V.Grid(nu=8, nv=4, v_lo=-0.5, v_hi=0.5, margin=0.0, min_visible=1)
    obj = np.array([[4.0, 0.1, 0.1, 0.5], [4.0, 0.2, 0.2, 0.5], [4.0, 0.3, 0.3, 0.5], [4.5, 0.1, 0.1, 0.5], [4.0, 0.15, 0.15, 0.5]], np.float32)
    none = np.zeros((0, 4), np.float32)
    want = _check(none, _far_boxes(3), obj, [0, 1, 4, 5], g)
    assert want["obj_keep"].tolist() == [True, True, True, False, True] and want["kept"].tolist() == [1, 2, 1]
    want = _check(none, _far_boxes(2), obj, [0, 4, 5], g)          # the farther point is the owner's own: it stays
    assert want["obj_keep"].all()
    want = _check(none, _far_boxes(2), obj[::-1].copy(), [0, 1, 5], g)
    assert want["obj_keep"].tolist() == [True, False, True, True, True]


def test_hand_made_scene_and_an_object_behind_another_one():
    g, scene, boxes, obj, off = hand_made_scene()
    want = _check(scene, boxes, obj, off, g)
    assert want["accepted"].tolist() == [True, False, True, False] and want["stats"][1] > 0
    second = car_face(14.0, 0.0, along_y=True)
    boxes2 = np.array([boxes[0], [16.0, 0.0, -1.75, 1.65, 1.6, 4.0, 0.0]])
    objs = [obj[:96], second]
    want = _check(scene[scene[:, 0] != 20.0], boxes2, np.concatenate(objs), V.offsets_of(objs), g)
    # culled by the nearer pasted car, still accepted: its label stays
    assert want["accepted"].all() and want["visible"].tolist() == [96, 96] and want["kept"][0] == 96 and 0 < want["kept"][1] < 96


def _frame_case(f=1):
    cloud, _ = _frame(f)
    es = [e for e in _ref_db() if len(e["points"]) >= 5][8 * f:8 * f + 8]
    objs = [e["points"] for e in es]
    return cloud, np.array([e["box"] for e in es]), np.concatenate(objs), V.offsets_of(objs)


def test_min_visible_extremes_margin_inf_and_cap():
    from voxelnet_amd import gtsample as G
    cloud, boxes, obj, off = _frame_case()
    cloud = np.array(cloud)
    cloud[[3, 700, 19000], [0, 1, 2]] = np.nan                      # NaN rows go whatever the thresholds
    want = _check(cloud, boxes, obj, off, V.Grid(min_visible=0))
    assert want["accepted"].all() and (want["visible"] == 0).any()          # accepted with nothing visible: its box still removes
    want = _check(cloud, boxes, obj, off, V.Grid(min_visible=10 ** 6))
    scene = cloud[~np.isnan(cloud[:, :3]).any(1)]
    assert not want["accepted"].any() and want["count"] == len(scene) == len(cloud) - 3
    assert np.array_equal(want["out"][:want["count"]], scene) and want["stats"].tolist() == [0, 0] and not want["kept"].any()
    # margin = inf, min_visible = 0: vn_gt_paste on the same inputs, bit for bit
    g = V.Grid(margin=np.inf, min_visible=0)
    out, count, visible, kept, stats, _ = _dev(cloud, boxes, obj, off, g)
    plain, plain_count = G.gt_paste_device(torch.from_numpy(cloud).to(DEV), _params(boxes, obj, off), padded=True)
    assert count == int(plain_count.item()) and _same(out, plain.cpu().numpy())
    assert np.array_equal(visible, np.diff(off)) and np.array_equal(kept, np.diff(off)) and stats[1] == 0
    _check(cloud, boxes, obj, off, g)
    # cap > n + m: NaN rows up to the end; the synchronising form is the buffer sliced to the count
    n_m = len(cloud) + len(obj)
    for cap in (n_m, n_m + 1, n_m + 1000):
        want = _check(cloud, boxes, obj, off, V.Grid(), cap)
        assert want["out"].shape == (cap, 4)
    sliced, k, res = G.gt_paste_visible_device(torch.from_numpy(cloud).to(DEV), _params(boxes, obj, off), _visibility(V.Grid()))
    assert k == want["count"] and _same(sliced.cpu().numpy(), want["out"][:k]) and np.array_equal(res.accepted, want["accepted"])
    with pytest.raises(Exception, match="invalid argument"):
        _dev(cloud, boxes, obj, off, V.Grid(), cap=n_m - 1)


def test_on_a_side_stream_the_counts_arrive_in_pinned_memory():
    from voxelnet_amd import gtsample as G
    cloud, boxes, obj, off = _frame_case(2)
    want = V.paste_visible(cloud, boxes, obj, off, V.Grid())
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        pts = torch.from_numpy(np.array(cloud)).pin_memory().to(DEV, non_blocking=True)
        out, keep, visible = G.enqueue_gt_paste_visible(pts, _params(boxes, obj, off), _visibility(V.Grid()))
    st.synchronize()
    assert visible.is_pinned() and not visible.is_cuda and any(t is visible for t in keep)
    assert np.array_equal(visible.numpy(), want["visible"]) and _same(out.cpu().numpy(), want["out"])


# ---------------------------------------------------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------------------------------------------------
def _make_kitti(root, frames):
    from PIL import Image
    for d in ("image_2", "velodyne", "label_2"):
        os.makedirs(os.path.join(root, d))
    for i, f in enumerate(frames):
        tag = f"{i:06d}"
        cloud, labels = _frame(f)
        np.ascontiguousarray(cloud, dtype=np.float32).tofile(os.path.join(root, "velodyne", tag + ".bin"))
        with open(os.path.join(root, "label_2", tag + ".txt"), "w") as fh:
            fh.write("\n".join(labels) + "\n")
        Image.fromarray(np.full((4, 6, 3), i, dtype=np.uint8)).save(os.path.join(root, "image_2", tag + ".png"))


def _read(root, tag):
    cloud = np.fromfile(os.path.join(root, "velodyne", tag + ".bin"), dtype=np.float32).reshape(-1, 4)
    return cloud, open(os.path.join(root, "label_2", tag + ".txt")).readlines()


def _loader(root):
    from voxelnet_amd import dataset as D
    ds = D.KITTIDataset(root, shuffle=False, augment=False, load_images=False)
    return torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=list, num_workers=0)


def _package_db():
    from voxelnet_amd import gtsample as G
    return G.GTDatabase([G.GTEntry(e["cls"], e["tag"], e["box"].copy(), e["points"].copy(), e["line"]) for e in _ref_db()])


def _same_batches(a, b):
    for x, y in zip(a, b):
        assert x[0] == y[0] and all(list(p) == list(q) for p, q in zip(x[1], y[1]))
        for j in (2, 3, 4):
            assert all(torch.equal(p, q) for p, q in zip(x[j], y[j]))
        assert all(np.array_equal(p, q) for p, q in zip(x[6], y[6]))
    assert len(a) == len(b)


SEED = 77


@pytest.mark.parametrize("augment", [False, True, "compose"])
def test_visibility_batcher_matches_the_host_replay(tmp_path, augment):
    """copy -> visible paste -> [augment | compose] -> voxelize against shuffle -> the restatement's draw -> the
    restatement's visible paste -> [the augmentation's restatement] -> oracle voxelizer; labels = labels + the accepted
    objects' lines (moved); the np.random state after the batches is that of visibility=None"""
    from voxelnet_amd import augment as A
    from voxelnet_amd import dataset as D
    from voxelnet_amd import gtsample as G
    root = str(tmp_path / "train")
    _make_kitti(root, [0, 1, 2])
    db, ref_db = _package_db(), list(_ref_db())
    aug = A.ComposeRecipe() if augment == "compose" else augment
    np.random.seed(SEED)
    plain = list(D.DeviceBatcher(_loader(root), DEV, "Car", augment=aug, gt_sampler=G.GTSampler(db, per_class=PER_CLASS)))
    tail_plain = np.random.random()
    np.random.seed(SEED)
    sampler = G.GTSampler(db, per_class=PER_CLASS, visibility=G.Visibility())
    batches = list(D.DeviceBatcher(_loader(root), DEV, "Car", augment=aug, gt_sampler=sampler))
    assert np.random.random() == tail_plain                      # the same random numbers with and without
    assert [len(b[0]) for b in batches] == [2, 1]
    np.random.seed(SEED)
    k = rejected = dropped_points = 0
    for (tags, label, feats, nums, coords, rgb, raw), other in zip(batches, plain):
        for i in range(len(tags)):
            tag = f"{k:06d}"
            assert tags[i] == tag
            cloud, lines = _read(root, tag)
            np.random.shuffle(cloud)
            assert np.array_equal(raw[i], cloud)                 # element 6: the host cloud as shuffled, as before
            d = R.draw(ref_db, lines, tag, PER_CLASS)
            enlarged = lines + d["lines"]
            off = V.offsets_of([e["points"] for line in d["lines"] for e in ref_db if e["line"] == line])
            assert off[-1] == len(d["points"]) and len(d["lines"]) >= 5
            want = V.paste_visible(cloud, d["boxes"], d["points"], off, V.Grid())
            pasted = want["out"][:want["count"]]
            acc = want["accepted"]
            rejected += int((~acc).sum())
            dropped_points += len(cloud) + len(d["points"]) - want["count"]
            print(f"sample {k}: {len(d['lines'])} candidates, {int((~acc).sum())} rejected, stats {want['stats'].tolist()}")
            if augment is True:
                state = np.random.get_state()
                da = AR.draw(enlarged)                           # on the lines of EVERY candidate
                np.random.set_state(state)
                moved_lines = A.augment_labels(enlarged, A.draw_augmentation(enlarged))
                pasted = AR.apply(pasted, da)
            elif augment == "compose":
                dc = CR.draw(enlarged, CR.recipe())
                pr = CR.to_params(dc["table"], dc["affine"])
                pr.boxes_after, pr.has_box = dc["after"], dc["has_box"]
                moved_lines = A.compose_labels(enlarged, pr)
                pasted = CR.apply(pasted, dc["table"], dc["affine"])
            else:
                moved_lines = enlarged
            assert len(moved_lines) == len(enlarged)
            keep_lines = moved_lines[:len(lines)] + [moved_lines[len(lines) + o] for o in range(len(acc)) if acc[o]]
            assert list(label[i]) == keep_lines
            assert len(other[1][i]) == len(enlarged)             # without visibility every candidate's line is there
            ref = ov.voxelize(pasted, "Car")
            assert np.array_equal(feats[i].cpu().numpy(), ref["feature_buffer"]), k
            assert np.array_equal(nums[i].cpu().numpy(), ref["number_buffer"]), k
            c = coords[i].cpu().numpy()
            assert np.array_equal(c[:, 1:], ref["coordinate_buffer"]) and (c[:, 0] == i).all()
            k += 1
    assert k == 3 and rejected >= 1 and dropped_points >= 30          # on the restatement alone: not vacuous
    assert np.random.random() == tail_plain


def test_visibility_none_is_the_pipeline_as_it_was(tmp_path, monkeypatch):
    """GTSampler(db) and GTSampler(db, visibility=None) give the same batches from the same launches: vn_gt_paste, never
    vn_gt_paste_visible; a sampler with a visibility calls vn_gt_paste_visible once per sample instead"""
    from voxelnet_amd import _lib
    from voxelnet_amd import dataset as D
    from voxelnet_amd import gtsample as G
    root = str(tmp_path / "kitti")
    _make_kitti(root, [0, 1, 2])
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    db = _package_db()
    runs = []
    for kw in ({}, {"visibility": None}):
        np.random.seed(7)
        del calls[:]
        batches = list(D.DeviceBatcher(_loader(root), DEV, "Car", gt_sampler=G.GTSampler(db, per_class=PER_CLASS, **kw)))
        runs.append((batches, np.random.random(), list(calls)))
    (a, ta, ca), (b, tb, cb) = runs
    assert ta == tb and ca == cb and ca.count("vn_gt_paste") == 3 and "vn_gt_paste_visible" not in ca
    _same_batches(a, b)
    # today's batch, replayed on the host
    np.random.seed(7)
    cloud, lines = _read(root, "000000")
    np.random.shuffle(cloud)
    d = R.draw(list(_ref_db()), lines, "000000", PER_CLASS)
    pasted, count = R.paste(cloud, d["boxes"], d["points"])
    ref = ov.voxelize(pasted[:count], "Car")
    assert list(a[0][1][0]) == lines + d["lines"] and np.array_equal(a[0][2][0].cpu().numpy(), ref["feature_buffer"])
    del calls[:]
    np.random.seed(7)
    list(D.DeviceBatcher(_loader(root), DEV, "Car", gt_sampler=G.GTSampler(db, per_class=PER_CLASS, visibility=G.Visibility())))
    assert calls.count("vn_gt_paste_visible") == 3 and "vn_gt_paste" not in calls and np.random.random() == ta
