"""GPU: the device half of the ground-truth database sampling — `vn_points_in_boxes` and `vn_gt_paste`
(csrc/gtsample.hip through voxelnet_amd.gtsample) against tests/gtsample_ref.py, BIT-EQUAL, the database cut on the
device against the restatement's, and the `gt_sampler=` switch of DeviceCollate / DeviceBatcher against a host replay of
the same shuffles and draws (voxel buffers = oracle voxelizer of the restatement's cloud, bit for bit)."""
import functools
import os

import numpy as np
import pytest
import torch

import augment_ref as AR
import gtsample_ref as R
from oracle import fov as of
from oracle import voxelize as ov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PER_CLASS = {"Car": 15}


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


def _params(boxes, obj):
    from voxelnet_amd import gtsample as G
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 7)
    return G.GTSampleParams(G.box_table(boxes), np.asarray(obj, dtype=np.float32).reshape(-1, 4), boxes, [])


def _dev_index(cloud, boxes, counts=True):
    from voxelnet_amd import gtsample as G
    pts = torch.from_numpy(np.array(cloud, dtype=np.float32)).to(DEV)
    index, cnt = G.points_in_boxes_device(pts, G.box_table(np.asarray(boxes, dtype=np.float64).reshape(-1, 7)), counts=counts)
    assert np.array_equal(pts.cpu().numpy(), cloud, equal_nan=True)
    return index.cpu().numpy(), (cnt.cpu().numpy() if counts else None)


def _dev_paste(cloud, boxes, obj, cap=None):
    from voxelnet_amd import gtsample as G
    pts = torch.from_numpy(np.array(cloud, dtype=np.float32)).to(DEV)
    out, count = G.gt_paste_device(pts, _params(boxes, obj), padded=True, cap=cap)
    assert np.array_equal(pts.cpu().numpy(), cloud, equal_nan=True)          # the input is left alone
    return out.cpu().numpy(), int(count.item())


def _check_all(cloud, boxes, obj, cap=None):
    """index (both kernels), counts and paste against the restatement -> (index, counts, out, count) of the restatement"""
    from voxelnet_amd import gtsample as G
    index, counts = R.index_counts(cloud, boxes)
    got_i, got_c = _dev_index(cloud, boxes)
    assert got_i.dtype == np.int32 and got_c.dtype == np.int32
    assert np.array_equal(got_i, index), int((got_i != index).sum())
    assert np.array_equal(got_c, counts), (got_c, counts)
    assert np.array_equal(_dev_index(cloud, boxes, counts=False)[0], index)
    want, count = R.paste(cloud, boxes, obj, cap)
    got, got_count = _dev_paste(cloud, boxes, obj, cap)
    assert got_count == count, (got_count, count)
    assert _same(got, want), int((got.view(np.uint32) != want.view(np.uint32)).any(1).sum())
    assert np.isnan(got[count:]).all()
    # the synchronising form is the same cloud sliced to the count
    pts = torch.from_numpy(np.array(cloud, dtype=np.float32)).to(DEV)
    assert _same(G.gt_paste_device(pts, _params(boxes, obj), cap=cap).cpu().numpy(), want[:count])
    return index, counts, want, count


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", range(4))
def test_synthetic_frames_are_bit_equal_to_the_restatement(f):
    """database of frames 8..23 pasted into frame f: ~19-20k points, 76+ workgroups, so the scan spans many counts"""
    cloud, labels = _frame(f)
    db = _ref_db()
    assert len(db) == 96 and sum(len(e["points"]) >= 5 for e in db) == 55
    np.random.seed(100 + f)
    d = R.draw(db, list(labels), f"{f:06d}", PER_CLASS)
    want, count = R.paste(cloud, d["boxes"], d["points"])
    removed, pasted = len(cloud) + len(d["points"]) - count, len(d["points"])
    print(f"frame {f}: {len(cloud)} points, {len(d['lines'])} objects accepted, {removed} removed, {pasted} pasted")
    assert len(cloud) > 76 * 256 - 256
    assert len(d["lines"]) >= 5 and removed >= 20 and pasted >= 20          # on the restatement alone: not vacuous
    _check_all(cloud, d["boxes"], d["points"])
    # determinism: a second run gives the same bits
    a, b = _dev_paste(cloud, d["boxes"], d["points"]), _dev_paste(cloud, d["boxes"], d["points"])
    assert a[1] == b[1] and _same(a[0], b[0])
    i0, c0 = _dev_index(cloud, d["boxes"])
    i1, c1 = _dev_index(cloud, d["boxes"])
    assert i0.tobytes() == i1.tobytes() and c0.tobytes() == c1.tobytes()


def _cubes(rng, g):
    """g 1.5 m cubes at random yaw over the crop"""
    return np.stack([rng.uniform(2, 68, g), rng.uniform(-38, 38, g), rng.uniform(-3, -0.5, g), np.full(g, 1.5), np.full(g, 1.5),
                     np.full(g, 1.5), rng.uniform(-np.pi / 2, np.pi / 2, g)], 1).reshape(g, 7)


def _cloud_near(rng, n, boxes):
    """n points: half of them within 1.5 m of a box centre (about a third of those inside), the rest anywhere"""
    pts = np.stack([rng.uniform(0, 70, n), rng.uniform(-40, 40, n), rng.uniform(-3, 1, n), np.round(rng.uniform(0, 1, n), 2)], 1)
    if len(boxes) and n:
        near = rng.random(n) < 0.5
        which = rng.integers(0, len(boxes), n)
        centre = boxes[which][:, :3] + np.array([0.0, 0.0, 0.75])
        pts[near, :3] = (centre + rng.uniform(-1.5, 1.5, (n, 3)))[near]
    return np.ascontiguousarray(pts, dtype=np.float32)


@pytest.mark.parametrize("n_boxes", [0, 1, 128])
def test_block_edges(n_boxes):
    rng = np.random.default_rng(7 + n_boxes)
    boxes = _cubes(rng, n_boxes)
    hit = 0
    # 65,535 ... 131,073: 256, 256, 257 and 513 workgroups — the one-workgroup scan takes 256 counts per trip, so its
    # carry starts at row 65,536 (with boxes only, and without m = 1)
    for n in (0, 1, 255, 256, 257, 1023, 1025, 65_535, 65_536, 65_537, 131_073):
        if n >= 65_535 and n_boxes == 0:
            continue
        for m in (0, 1, 300) if n < 65_535 else (0, 300):
            cloud = _cloud_near(rng, n, boxes)
            obj = _cloud_near(rng, m, boxes[:0])
            index, counts, _, count = _check_all(cloud, boxes, obj)
            assert counts.shape == (n_boxes,) and count <= n + m
            hit += int((index >= 0).sum())
            if n >= 65_535:                      # on the restatement alone: kept rows on both sides of row 65,536
                kept = index < 0
                assert kept[:65_536].any() and 0 < count - m < n
                assert n <= 65_536 or kept[65_536:].any()
    assert hit >= (300 if n_boxes else 0)                          # the boxes do take points away
    # cap exactly n + m and larger; rows past the count are NaN
    cloud, obj = _cloud_near(rng, 1025, boxes), _cloud_near(rng, 300, boxes[:0])
    for cap in (1325, 1326, 2048, 5000):
        _, _, want, count = _check_all(cloud, boxes, obj, cap)
        assert want.shape == (cap, 4) and count <= 1325


def test_all_points_inside_one_box_and_no_point_inside_any():
    rng = np.random.default_rng(3)
    box = np.array([[30.0, 5.0, -2.0, 2.0, 3.0, 5.0, 0.4]])
    c, s = np.cos(0.4), np.sin(0.4)
    u, v = rng.uniform(-2.4, 2.4, 700), rng.uniform(-1.4, 1.4, 700)
    inside = np.stack([30.0 + u * c - v * s, 5.0 + u * s + v * c, rng.uniform(-1.9, -0.1, 700), np.full(700, 0.25)], 1).astype(np.float32)
    obj = _cloud_near(rng, 40, box[:0])
    assert R.inside(inside, box[0]).all()
    _, counts, want, count = _check_all(inside, box, obj)          # k = 0: the objects start at row 0
    assert counts.tolist() == [700] and count == 40 and np.array_equal(want[:40], obj)
    _check_all(inside, box, obj[:0])                               # ... and nothing at all comes out
    far = inside + np.float32([100.0, 0.0, 0.0, 0.0])
    index, counts, want, count = _check_all(far, np.concatenate([box, _cubes(rng, 127)]), obj)
    assert (index == -1).all() and not counts.any() and count == 740 and np.array_equal(want[:700], far)


def test_status_codes_on_device_buffers():
    from voxelnet_amd import _lib
    from voxelnet_amd import gtsample as G
    cloud = torch.from_numpy(_cloud_near(np.random.default_rng(0), 600, np.zeros((0, 7)))).to(DEV)
    obj = np.zeros((10, 4), np.float32)
    with pytest.raises(_lib.VoxelnetHipError, match="invalid argument"):
        G.gt_paste_device(cloud, _params([], obj), cap=609)                    # cap < n + m
    with pytest.raises(_lib.VoxelnetHipError):
        G.gt_paste_device(cloud, _params(np.zeros((129, 7)), obj))             # 129 table entries
    with pytest.raises(_lib.VoxelnetHipError):
        G.points_in_boxes_device(cloud, G.box_table(np.zeros((129, 7))))
    for bad in (cloud.cpu(), cloud[:, :3], cloud.double(), cloud[::2]):
        with pytest.raises(_lib.VoxelnetHipError):
            G.gt_paste_device(bad, _params([], obj))
        with pytest.raises(_lib.VoxelnetHipError):
            G.points_in_boxes_device(bad, G.box_table(np.zeros((1, 7))))
    # a 4-byte-offset pointer, straight at the C ABI
    lib = _lib.load()
    flat = torch.zeros(4 * 700 + 4, dtype=torch.float32, device=DEV)
    out = torch.empty((700, 4), dtype=torch.float32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.vn_gt_paste_workspace_bytes(600), dtype=torch.uint8, device=DEV)
    index = torch.empty(600, dtype=torch.int32, device=DEV)
    st = _lib.raw_stream()
    assert lib.vn_gt_paste(flat.data_ptr() + 4, 600, None, 0, None, 0, out.data_ptr(), 700, count.data_ptr(), ws.data_ptr(),
                           ws.numel(), st) == -2
    assert lib.vn_gt_paste(cloud.data_ptr(), 600, None, 0, None, 0, flat.data_ptr() + 4, 600, count.data_ptr(), ws.data_ptr(),
                           ws.numel(), st) == -2
    assert lib.vn_gt_paste(cloud.data_ptr(), 600, None, 0, None, 0, out.data_ptr(), 599, count.data_ptr(), ws.data_ptr(),
                           ws.numel(), st) == -1
    assert lib.vn_gt_paste(cloud.data_ptr(), 600, None, 0, None, 0, cloud.data_ptr(), 600, count.data_ptr(), ws.data_ptr(),
                           ws.numel(), st) == -1                                # out must not be the input
    assert lib.vn_gt_paste(cloud.data_ptr(), 600, None, 0, None, 0, out.data_ptr(), 700, count.data_ptr(), ws.data_ptr(),
                           ws.numel() - 257, st) == -3
    assert lib.vn_points_in_boxes(flat.data_ptr() + 4, 600, None, 0, index.data_ptr(), None, st) == -2
    torch.cuda.synchronize()


def test_a_hand_made_dense_frame():
    """2,000 points inside a 4 x 1.6 x 1.5 m box at r = 0.6 plus 2,000 around it; a second box that overlaps the first"""
    rng = np.random.default_rng(11)
    box = np.array([25.0, -6.0, -1.8, 1.5, 1.6, 4.0, 0.6])
    c, s = np.cos(0.6), np.sin(0.6)

    def place(u, v, z):
        return np.stack([25.0 + u * c - v * s, -6.0 + u * s + v * c, z, np.round(rng.uniform(0, 1, len(u)), 2)], 1).astype(np.float32)
    inner = place(rng.uniform(-2, 2, 2000), rng.uniform(-0.8, 0.8, 2000), rng.uniform(-1.8, -0.3, 2000))
    outer = place(rng.uniform(-5, 5, 2000), rng.uniform(-4, 4, 2000), rng.uniform(-3.0, 1.0, 2000))
    cloud = np.concatenate([inner, outer])[rng.permutation(4000)]
    obj = place(rng.uniform(-1, 1, 150), rng.uniform(-0.5, 0.5, 150), rng.uniform(-1.5, -0.5, 150)) + np.float32([0, 20, 0, 0])
    index, counts, _, count = _check_all(cloud, box[None], obj)
    assert 1950 <= counts[0] < 2400 and (index == 0).sum() == counts[0] and count == 4150 - counts[0]
    second = np.array([26.5, -5.0, -2.0, 1.5, 1.6, 4.0, -0.3])
    both = np.stack([box, second])
    index, counts, _, _ = _check_all(cloud, both, obj)
    assert counts[1] > 100 and counts.sum() > (index >= 0).sum() > counts[0]          # shared points count for both
    # the table's order decides the index, not the counts
    index_r, counts_r, _, _ = _check_all(cloud, both[::-1], obj)
    assert counts_r.tolist() == counts[::-1].tolist() and (index_r == 0).sum() == counts[1]


def test_nan_padding_goes_and_comes_back(golden):
    """a cloud whose tail is fov_crop_device(..., padded=True) padding: the padding is dropped from the middle (between
    the scene rows and the pasted rows) and re-created at the end"""
    from voxelnet_amd import gtsample as G
    from voxelnet_amd.fov import fov_crop_device
    g = golden("fov_crop")
    rows, cols = (int(v) for v in g["image_shape"])
    frame, labels = _frame(1)
    rng = np.random.default_rng(5)
    extra = np.stack([rng.uniform(-70, 70, 9000), rng.uniform(-40, 40, 9000), rng.uniform(-3, 1, 9000),
                      np.round(rng.uniform(0, 1, 9000), 2)], 1).astype(np.float32)
    raw = np.concatenate([frame, extra])[rng.permutation(len(frame) + 9000)]
    kept, _ = of.fov_crop(raw, g["P"], g["Tr"], g["R"], rows, cols)
    padded, cnt = fov_crop_device(torch.from_numpy(raw).to(DEV), g["P"], g["Tr"], g["R"], rows, cols, padded=True)
    assert padded.shape[0] == len(raw) and 0 < int(cnt.item()) == len(kept) < len(raw)
    np.random.seed(21)
    d = R.draw(_ref_db(), list(labels), "000001", PER_CLASS)
    assert len(d["lines"]) >= 5
    want, count = R.paste(kept, d["boxes"], d["points"], cap=len(raw) + len(d["points"]))
    out, dev_count = G.gt_paste_device(padded, _params(d["boxes"], d["points"]), padded=True)
    assert int(dev_count.item()) == count < len(kept) + len(d["points"])
    assert _same(out.cpu().numpy(), want) and np.isnan(want[count:]).all()
    assert np.array_equal(want[count - len(d["points"]):count], d["points"])
    # NaN rows anywhere: a padded buffer followed by real points, and a row with one NaN coordinate only
    mixed = np.concatenate([padded.cpu().numpy(), frame[:3000]])
    mixed[5, 1] = np.nan
    mixed[6, 2] = np.nan
    j = 7 + int(np.argmin(R.masks(mixed[7:200], d["boxes"]).any(0)))          # a scene row that lies in no box
    mixed[j, 3] = np.nan                                            # reflectance is no coordinate: the row stays
    _, _, want, count = _check_all(mixed, d["boxes"], d["points"])
    assert np.isnan(want[:count, :3]).sum() == 0 and np.isnan(want[:count, 3]).sum() == 1


def test_on_a_side_stream_without_host_synchronisation():
    from voxelnet_amd import gtsample as G
    cloud, labels = _frame(2)
    np.random.seed(8)
    d = R.draw(_ref_db(), list(labels), "000002", PER_CLASS)
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        pts = torch.from_numpy(np.array(cloud)).pin_memory().to(DEV, non_blocking=True)
        out, keep = G.enqueue_gt_paste(pts, _params(d["boxes"], d["points"]))
    st.synchronize()
    want, _ = R.paste(cloud, d["boxes"], d["points"])
    assert _same(out.cpu().numpy(), want) and len(keep) >= 5


def test_dense_workload_cloud():
    """config 5's frame (~300k points, > 1024 workgroups: the one-workgroup scan makes five trips of 256 counts), 32 boxes"""
    from voxelnet_amd import synth
    cloud = synth.workload_frames(5, batch=1)[0]
    assert cloud.shape[0] > 262144
    rng = np.random.default_rng(2)
    boxes = _cubes(rng, 32)
    boxes[:, 3:6] = [1.6, 1.7, 4.0]
    index, counts, _, count = _check_all(cloud, boxes, _frame(0)[0][:5000])
    assert (index >= 0).sum() >= 1000 and count < cloud.shape[0] + 5000 - 1000


# ---------------------------------------------------------------------------------------------------------------------
# database
# ---------------------------------------------------------------------------------------------------------------------
def _check_db(db, ref):
    assert len(db) == len(ref)
    for e, r in zip(db.entries, ref):
        assert (e.cls, e.tag, e.line) == (r["cls"], r["tag"], r["line"])
        assert e.box.tobytes() == r["box"].tobytes()
        assert e.points.dtype == np.float32 and e.points.shape == r["points"].shape and e.points.tobytes() == r["points"].tobytes()


def test_database_on_the_device_is_the_restatements(tmp_path):
    from voxelnet_amd import gtsample as G
    frames = [(f"{f:06d}", np.array(_frame(f)[0]), list(_frame(f)[1])) for f in range(8, 24)]
    db = G.GTDatabase.build(frames, DEV, classes=("Car",))
    _check_db(db, _ref_db())
    assert sum(e.points.shape[0] == 0 for e in db.entries) >= 1          # entries with 0 points are stored
    assert len(G.GTDatabase.build(frames[:2], DEV, classes=("Pedestrian",))) == 0          # the type must match exactly
    # overlapping boxes each keep their points: two label lines that share a region
    from voxelnet_amd.targets import lidar_box_to_label_line
    cloud = np.array(_frame(8)[0])
    centre = cloud[np.argmax((cloud[:, 2] > -2.5) & (cloud[:, 2] < -0.5) & (cloud[:, 0] > 10) & (cloud[:, 0] < 30))]
    lines = [lidar_box_to_label_line("Car", [centre[0], centre[1], -3.0, 3.0, 6.0, 8.0, 0.3]),
             lidar_box_to_label_line("Van", [centre[0] + 2.0, centre[1] + 1.0, -3.0, 3.0, 6.0, 8.0, -0.4]), "DontCare 0 0 0 0 0 0 0 1 1 1 0 0 0 0"]
    ref = R.database([("t", cloud, lines)], classes=("Car", "Van"))
    shared = R.inside(cloud, ref[0]["box"]) & R.inside(cloud, ref[1]["box"])
    assert len(ref) == 2 and shared.sum() >= 20 and len(ref[1]["points"]) > shared.sum()
    db2 = G.GTDatabase.build([("t", torch.from_numpy(cloud).to(DEV), lines)], DEV, classes=("Car", "Van"))
    _check_db(db2, ref)
    # and the round trip of what the device cut
    path = str(tmp_path / "db.npz")
    db.save(path)
    _check_db(G.GTDatabase.load(path), _ref_db())


# ---------------------------------------------------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------------------------------------------------
def _make_kitti(root, frames, first_tag, calib=None):
    """a throw-away KITTI directory (as tests/test_gpu_augment._make_kitti) of the synthetic frames `frames`"""
    from PIL import Image
    for d in ("image_2", "velodyne", "label_2") + (("calib",) if calib is not None else ()):
        os.makedirs(os.path.join(root, d))
    for i, f in enumerate(frames):
        tag = f"{first_tag + i:06d}"
        cloud, labels = _frame(f)
        if calib is not None:                    # a raw sweep: points all round the car, reflectance 0 now and then
            rng = np.random.default_rng(40 + f)
            extra = np.stack([rng.uniform(-70, 70, 20000), rng.uniform(-40, 40, 20000), rng.uniform(-3, 1, 20000),
                              np.round(rng.uniform(0, 1, 20000), 2)], 1).astype(np.float32)
            cloud = np.concatenate([cloud, extra])[rng.permutation(len(cloud) + 20000)]
            with open(os.path.join(root, "calib", tag + ".txt"), "w") as fh:
                def fmt(name, a):
                    return name + ": " + " ".join(f"{v:.12e}" for v in np.asarray(a).reshape(-1))
                fh.write("\n".join([fmt("P0", calib["P"]), fmt("P1", calib["P"]), fmt("P2", calib["P"]), fmt("P3", calib["P"]),
                                    fmt("R0_rect", calib["R"][:3, :3]), fmt("Tr_velo_to_cam", calib["Tr"][:3]),
                                    fmt("Tr_imu_to_velo", calib["Tr"][:3])]) + "\n")
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


@pytest.mark.parametrize("augment,fov", [(False, False), (True, False), (False, True), (True, True)])
def test_pasting_batcher_matches_the_host_replay(tmp_path, golden, augment, fov):
    """copy -> [crop] -> paste -> [augment] -> voxelize against shuffle -> the restatement's draws -> [oracle crop] ->
    the restatement's paste -> [the augmentation's restatement] -> oracle voxelizer; the database is cut on the device
    from a second directory (other tags) through the same crop"""
    from voxelnet_amd import augment as A
    from voxelnet_amd import dataset as D
    from voxelnet_amd import gtsample as G
    from voxelnet_amd.fov import load_calib
    g = golden("fov_crop")
    rows, cols = (int(v) for v in g["image_shape"])
    train, source = str(tmp_path / "train"), str(tmp_path / "source")
    _make_kitti(train, [0, 1, 2], 0, calib=g if fov else None)
    _make_kitti(source, range(8, 18), 100, calib=g if fov else None)
    kw = dict(fov_calib_dir=os.path.join(train, "calib"), image_shape=(rows, cols)) if fov else {}

    def crop(root, cloud, tag):
        if not fov:
            return cloud
        P, Tr, Rr = load_calib(os.path.join(root, "calib", tag + ".txt"))
        kept, _ = of.fov_crop(cloud, P, Tr, Rr, rows, cols)
        assert 0 < kept.shape[0] < cloud.shape[0]
        return kept
    src_ds = D.KITTIDataset(source, shuffle=False, load_images=False)
    db = G.GTDatabase.build_from_dataset(src_ds, DEV, ("Car",), fov_calib_dir=os.path.join(source, "calib") if fov else None,
                                         image_shape=(rows, cols))
    ref_db = R.database([(f"{t:06d}", crop(source, _read(source, f"{t:06d}")[0], f"{t:06d}"), _read(source, f"{t:06d}")[1])
                         for t in range(100, 110)])
    _check_db(db, ref_db)
    assert len(ref_db) == 60 and sum(len(e["points"]) >= 5 for e in ref_db) >= 20

    np.random.seed(77)
    sampler = G.GTSampler(db, per_class=PER_CLASS, min_points=5)
    batches = list(D.DeviceBatcher(_loader(train), DEV, "Car", augment=augment, gt_sampler=sampler, **kw))
    assert [len(b[0]) for b in batches] == [2, 1]
    np.random.seed(77)
    k = 0
    for tags, label, feats, nums, coords, rgb, raw in batches:
        assert isinstance(label, np.ndarray) and label.dtype == object and len(label) == len(tags)
        for i in range(len(tags)):
            tag = f"{k:06d}"
            assert tags[i] == tag
            cloud, lines = _read(train, tag)
            np.random.shuffle(cloud)
            d = R.draw(ref_db, lines, tag, PER_CLASS)
            enlarged = lines + d["lines"]
            assert np.array_equal(raw[i], cloud)                # raw lidar: the host cloud as shuffled
            base = crop(train, cloud, tag)
            pasted, count = R.paste(base, d["boxes"], d["points"])
            pasted = pasted[:count]
            removed = len(base) + len(d["points"]) - count
            print(f"sample {k}: {len(d['lines'])} accepted, {removed} removed, {len(d['points'])} pasted")
            assert len(d["lines"]) >= 3 and removed >= 10 and len(d["points"]) >= 20
            if augment:
                state = np.random.get_state()
                da = AR.draw(enlarged)                          # the augmentation's draw runs on the enlarged labels
                np.random.set_state(state)
                p = A.draw_augmentation(enlarged)
                assert np.array_equal(p.boxes_after, da["after"]) and len(da["after"]) == len(enlarged)
                assert list(label[i]) == A.augment_labels(enlarged, p)
                pasted = AR.apply(pasted, da)
            else:
                assert list(label[i]) == enlarged
            ref = ov.voxelize(pasted, "Car")
            assert np.array_equal(feats[i].cpu().numpy(), ref["feature_buffer"]), k
            assert np.array_equal(nums[i].cpu().numpy(), ref["number_buffer"]), k
            c = coords[i].cpu().numpy()
            assert np.array_equal(c[:, 1:], ref["coordinate_buffer"]) and (c[:, 0] == i).all()
            k += 1
    assert k == 3


def test_gt_sampler_none_is_the_pipeline_as_it_was(tmp_path, monkeypatch):
    """gt_sampler=None equals omitting the argument: same np.random consumption as a replay of the shuffles, same
    outputs, the new entry points never called; a sampler that accepts nothing gives the same voxel buffers without a
    launch; DeviceCollate takes the keyword too and then does call the paste"""
    from voxelnet_amd import _lib
    from voxelnet_amd import dataset as D
    from voxelnet_amd import gtsample as G
    root = str(tmp_path / "kitti")
    _make_kitti(root, [0, 1, 2], 0)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    db = G.GTDatabase([G.GTEntry(e["cls"], e["tag"], e["box"], e["points"], e["line"]) for e in _ref_db()])
    nothing = G.GTSampler(db, per_class={"Car": 6})                # six cars are there already
    runs = []
    for kw in ({}, {"gt_sampler": None}, {"gt_sampler": nothing}):
        np.random.seed(7)
        batches = list(D.DeviceBatcher(_loader(root), DEV, "Car", **kw))
        runs.append((batches, np.random.random()))
    assert "vn_gt_paste" not in calls and "vn_points_in_boxes" not in calls and "vn_voxelize_index" in calls
    np.random.seed(7)
    for k in range(3):
        np.random.shuffle(_read(root, f"{k:06d}")[0])
    today = np.random.random()
    (a, ta), (b, tb), (c, tc) = runs
    assert ta == tb == tc == today
    for other in (b, c):
        for x, y in zip(a, other):
            assert x[0] == y[0] and all(list(p) == list(q) for p, q in zip(x[1], y[1]))
            for j in (2, 3, 4):
                assert all(torch.equal(p, q) for p, q in zip(x[j], y[j]))
            assert all(np.array_equal(p, q) for p, q in zip(x[6], y[6]))
    assert list(a[0][1][0]) == _read(root, "000000")[1]
    # DeviceCollate with the keyword: the paste is called, labels grow, the voxel buffers are the replay's
    sampler = G.GTSampler(db, per_class=PER_CLASS)
    parts = list(_loader(root))[0]
    np.random.seed(9)
    tags, label, feats, nums, coords, _, raw = D.DeviceCollate(DEV, "Car", gt_sampler=sampler)(parts)
    assert calls.count("vn_gt_paste") == 2
    np.random.seed(9)
    for i in range(2):
        cloud, lines = _read(root, f"{i:06d}")
        np.random.shuffle(cloud)
        d = R.draw(_ref_db(), lines, f"{i:06d}", PER_CLASS)
        assert len(d["lines"]) >= 5 and list(label[i]) == lines + d["lines"]
        pasted, count = R.paste(cloud, d["boxes"], d["points"])
        ref = ov.voxelize(pasted[:count], "Car")
        assert np.array_equal(feats[i].cpu().numpy(), ref["feature_buffer"])
        assert np.array_equal(nums[i].cpu().numpy(), ref["number_buffer"])
        assert np.array_equal(coords[i].cpu().numpy()[:, 1:], ref["coordinate_buffer"])


def test_targets_see_the_pasted_boxes():
    """the device target generator on the enlarged labels is the oracle's on the enlarged labels, and marks positive
    anchors at pasted boxes that the original labels do not.  (The reference's anchor rectangle is the single point
    (x - l/2, y - w/2) of the anchor and its IoU adds one to every extent — oracle/targets.py — so a box's positive
    anchors have that point inside the box's hull grown by 1 m: at most 2.3 + 1 + 1.95 m from the centre on an axis;
    and its best anchor may be one that is positive already, so not every pasted box adds one.)"""
    from oracle import targets as ot
    from voxelnet_amd import gtsample as G
    from voxelnet_amd import targets as T
    _, labels = _frame(0)
    db = G.GTDatabase([G.GTEntry(e["cls"], e["tag"], e["box"], e["points"], e["line"]) for e in _ref_db()])
    np.random.seed(100)
    params = G.GTSampler(db, per_class=PER_CLASS).draw(list(labels), "000000")
    assert len(params.lines) >= 5
    enlarged = list(labels) + params.lines
    gen = T.TargetGenerator("Car", DEV)
    pos0 = gen([list(labels)])[0][0].cpu().numpy()
    pos1 = gen([enlarged])[0][0].cpu().numpy()
    anchors = T.generate_anchors("Car")
    want = ot.generate_targets([enlarged], anchors.shape[:2], anchors, "Car")[0][0]
    assert np.array_equal(pos1, want.astype(np.float32))
    new = (pos1 > 0) & (pos0 == 0)
    assert (pos1 >= pos0).all() and new.sum() >= 1
    at_a_box = np.zeros_like(new)
    gained = 0
    for box in params.boxes:
        near = (np.abs(anchors[..., 0] - box[0]) < 5.25) & (np.abs(anchors[..., 1] - box[1]) < 5.25)
        at_a_box |= near
        gained += bool(new[near].any())
    assert gained >= 1 and not (new & ~at_a_box).any()          # new positives sit at pasted boxes, nowhere else
