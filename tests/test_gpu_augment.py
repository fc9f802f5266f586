"""GPU: the device half of the augmentation — `vn_augment_points` (csrc/augment.hip through voxelnet_amd.augment) against
tests/augment_ref.py, BIT-EQUAL in each mode, and the `augment=True` switch of DeviceCollate / DeviceBatcher against a
host replay of the same shuffles and draws (voxel buffers = oracle voxelizer of the restatement's cloud, bit for bit)."""
import os

import numpy as np
import pytest
import torch

import augment_ref as R
from oracle import fov as of
from oracle import voxelize as ov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODE_OF = {"scale": lambda c: c < 4, "rotate": lambda c: 4 <= c < 7, "boxes": lambda c: c >= 7}


def _frame(f):
    from voxelnet_amd import synth
    return synth.synth_cloud("Car", 6000, synth.frame_seed(2, f), 2.3, 35), synth.synth_labels("Car", 6, f)


def _draw(labels, mode, start=0):
    """the package's draw under the first seed >= start whose choice selects `mode`"""
    from voxelnet_amd import augment as A
    for seed in range(start, start + 1000):
        np.random.seed(seed)
        if MODE_OF[mode](np.random.randint(0, 10)):
            np.random.seed(seed)
            p = A.draw_augmentation(labels)
            assert p.mode == mode
            return p
    raise AssertionError("no seed found")


def _same(a, b):
    """bit-equal float32 arrays (NaN rows: NaN in the same places — a NaN's payload is not part of the contract)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def _device(cloud, params, inplace=False):
    from voxelnet_amd import augment as A
    pts = torch.from_numpy(np.ascontiguousarray(cloud)).to(DEV)
    if inplace:
        out = A.augment_points_device(pts, params, out=pts)
        assert out is pts
    else:
        out = A.augment_points_device(pts, params)
        assert out is not pts and np.array_equal(pts.cpu().numpy(), cloud)          # the input is left alone
    return out.cpu().numpy()


@pytest.mark.parametrize("mode", ["boxes", "rotate", "scale"])
def test_kernel_is_bit_equal_to_the_restatement(mode):
    for f in range(4):
        cloud, labels = _frame(f)
        p = _draw(labels, mode, start=100 * f)
        want = R.apply(cloud, R.from_params(p))
        changed = int((want.view(np.uint32) != cloud.view(np.uint32)).any(1).sum())
        print(f"frame {f} {mode}: {changed} of {len(cloud)} points change")
        if mode == "boxes":
            assert len(p.table) == 7 and changed >= 20, (f, changed)       # six cars hold points; cannot pass vacuously
        else:
            assert changed > 0.9 * len(cloud)
        assert np.array_equal(want[:, 3], cloud[:, 3])                      # reflectance is never touched
        for inplace in (False, True):
            got = _device(cloud, p, inplace)
            assert _same(got, want), (f, mode, inplace, int((got.view(np.uint32) != want.view(np.uint32)).any(1).sum()))


def _manual(rows):
    from voxelnet_amd import augment as A
    table = np.zeros(len(rows), dtype=A.BOX_DTYPE)
    for i, (lo, hi, t, rz) in enumerate(rows):
        table[i] = (np.float32(lo), np.float32(hi), t, np.cos(rz), np.sin(rz))
    z = np.zeros((0, 7))
    return A.AugmentParams("boxes", 9, z, z, table=table)


def test_a_point_moved_into_a_later_box_is_moved_again():
    """box 0 = [0,1]^3 pushes its points 1 m along x (and turns them a little) into box 1 = [0.8,2.2] x [-1,1] x [0,1],
    which lifts them by 5 m: the walk is on the CURRENT value, in index order (the reference's in-place loop)"""
    rng = np.random.default_rng(0)
    cloud = np.concatenate([rng.uniform(0, 1, (500, 4)), rng.uniform(3, 9, (500, 4))]).astype(np.float32)
    p = _manual([((0, 0, 0), (1, 1, 1), (1.0, 0.0, 0.0), 0.05), ((0.8, -1, 0), (2.2, 1, 1), (0.0, 0.0, 5.0), -0.1)])
    want = R.apply(cloud, R.from_params(p))
    first = R.apply(cloud, dict(mode="boxes", table=R.from_params(p)["table"][:1]))
    twice = (first[:, 0] != cloud[:, 0]) & (want[:, 2] != first[:, 2])
    assert twice.sum() >= 400 and (want[twice, 2] > 4.9).all()
    assert np.array_equal(want[500:], cloud[500:])
    for inplace in (False, True):
        assert _same(_device(cloud, p, inplace), want)
    # reversed table: box 1 first catches nothing of the unit cube's points with x < 0.8, so the result differs
    q = _manual([((0.8, -1, 0), (2.2, 1, 1), (0.0, 0.0, 5.0), -0.1), ((0, 0, 0), (1, 1, 1), (1.0, 0.0, 0.0), 0.05)])
    want_q = R.apply(cloud, R.from_params(q))
    assert not np.array_equal(want_q, want) and _same(_device(cloud, q), want_q)


def test_table_sizes_empty_cloud_and_bounds_edges():
    from voxelnet_amd import _lib
    from voxelnet_amd import augment as A
    cloud, labels = _frame(0)
    # 0 boxes: nothing moves, out of place is a copy
    p0 = _manual([])
    for inplace in (False, True):
        assert _same(_device(cloud, p0, inplace), cloud)
    # a label without any line in boxes mode
    assert _same(_device(cloud, _draw([], "boxes")), cloud)
    # 128 boxes (the table's capacity, 8 KB of LDS): 1.5 m cubes scattered over the crop
    rng = np.random.default_rng(1)
    rows = []
    for _ in range(A.MAX_BOXES):
        lo = np.array([rng.uniform(0, 68), rng.uniform(-40, 38), rng.uniform(-3, 0)])
        rows.append((lo, lo + 1.5, tuple(rng.normal(size=3)), rng.uniform(-np.pi / 10, np.pi / 10)))
    p128 = _manual(rows)
    want = R.apply(cloud, R.from_params(p128))
    assert (want != cloud).any(1).sum() > 300
    for inplace in (False, True):
        assert _same(_device(cloud, p128, inplace), want)
    with pytest.raises(_lib.VoxelnetHipError):
        _device(cloud, _manual(rows + rows[:1]))                                        # 129 entries
    # n = 0 in every mode
    for mode in ("boxes", "rotate", "scale"):
        out = A.augment_points_device(torch.empty((0, 4), dtype=torch.float32, device=DEV), _draw(labels, mode))
        assert out.shape == (0, 4)
    # the comparison is inclusive and float32: points exactly on lo / hi move, their float32 neighbours outside do not
    lo, hi = np.float32([1.1, -2.3, 0.7]), np.float32([3.3, 0.1, 1.9])
    edge = np.array([[lo[0], lo[1], lo[2], 0.5], [hi[0], hi[1], hi[2], 0.5], [np.nextafter(lo[0], np.float32(-9)), lo[1], lo[2], 0.5],
                     [hi[0], np.nextafter(hi[1], np.float32(9)), hi[2], 0.5], [hi[0], hi[1], np.nextafter(hi[2], np.float32(9)), 0.5]], np.float32)
    pe = _manual([(lo, hi, (0.25, -0.5, 1.0), 0.2)])
    want = R.apply(edge, R.from_params(pe))
    assert (want[:2] != edge[:2]).any(1).all() and np.array_equal(want[2:], edge[2:])
    assert _same(_device(edge, pe), want)
    # wrong inputs: no CPU path, shape, dtype, layout
    p = _draw(labels, "rotate")
    pts = torch.from_numpy(cloud).to(DEV)
    for bad in (torch.from_numpy(cloud), pts[:, :3], pts.double(), pts[::2]):
        with pytest.raises(_lib.VoxelnetHipError):
            A.augment_points_device(bad, p)
    with pytest.raises(_lib.VoxelnetHipError):
        A.augment_points_device(pts, p, out=torch.empty((5, 4), device=DEV))


def test_on_a_side_stream_without_host_synchronisation():
    """enqueued on the CURRENT stream (a non-default one here), ordered behind the upload on that stream"""
    from voxelnet_amd import augment as A
    cloud, labels = _frame(1)
    st = torch.cuda.Stream(device=DEV)
    outs = []
    with torch.cuda.stream(st):
        for mode in ("boxes", "rotate", "scale"):
            p = _draw(labels, mode)
            pts = torch.from_numpy(cloud).pin_memory().to(DEV, non_blocking=True)
            outs.append((p, A.augment_points_device(pts, p, out=pts)))
    st.synchronize()
    for p, out in outs:
        assert _same(out.cpu().numpy(), R.apply(cloud, R.from_params(p)))


def test_nan_padding_rows_stay_nan():
    """the padded field-of-view crop's tail rows are NaN points: untouched by boxes mode, NaN after the other two, and
    the rows in front of them are moved as usual"""
    cloud, labels = _frame(2)
    padded = cloud.copy()
    padded[-1500:] = np.nan
    for mode in ("boxes", "rotate", "scale"):
        p = _draw(labels, mode)
        got = _device(padded, p, inplace=True)
        assert np.isnan(got[-1500:, :3]).all()
        assert _same(got[:-1500], R.apply(cloud[:-1500], R.from_params(p)))
        assert _same(got, R.apply(padded, R.from_params(p)))


def test_dense_workload_cloud():
    """config 5's frame (~300k points), 16 cars"""
    from voxelnet_amd import synth
    cloud = synth.workload_frames(5, batch=1)[0]
    assert cloud.shape[0] > 250_000
    labels = synth.synth_labels("Car", 16, 3)
    for mode in ("boxes", "rotate", "scale"):
        p = _draw(labels, mode)
        want = R.apply(cloud, R.from_params(p))
        if mode == "boxes":
            assert (want != cloud).any(1).sum() >= 1000
        assert _same(_device(cloud, p, inplace=True), want)


# ---------------------------------------------------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------------------------------------------------
def _make_kitti(root, n, calib=None):
    """a throw-away KITTI directory (as tests/test_gpu_dataset._make_kitti) of the frames above: cars with points inside"""
    from PIL import Image
    for d in ("image_2", "velodyne", "label_2") + (("calib",) if calib is not None else ()):
        os.makedirs(os.path.join(root, d))
    for i in range(n):
        tag = f"{i:06d}"
        cloud, labels = _frame(i % 4)
        if calib is not None:                    # a raw sweep: points all round the car, reflectance 0 now and then
            rng = np.random.default_rng(40 + i)
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


def _check_batches(root, batches, crop=None):
    """replays the shuffles and the draws on the host (the np.random seed is the caller's) and checks every sample"""
    from voxelnet_amd import augment as A
    modes, k = [], 0
    for b in batches:
        tags, label, feats, nums, coords, rgb, raw = b
        assert isinstance(label, np.ndarray) and label.dtype == object and len(label) == len(tags)
        for i in range(len(tags)):
            cloud = np.fromfile(os.path.join(root, "velodyne", f"{k:06d}.bin"), dtype=np.float32).reshape(-1, 4)
            lines = open(os.path.join(root, "label_2", f"{k:06d}.txt")).readlines()
            np.random.shuffle(cloud)
            state = np.random.get_state()
            d = R.draw(lines)                                   # the restatement's draw ...
            np.random.set_state(state)
            p = A.draw_augmentation(lines)                      # ... and the package's, from the same stream position
            modes.append(d["mode"])
            assert np.array_equal(raw[i], cloud)                # raw lidar: the host cloud as shuffled, un-augmented
            assert list(label[i]) == A.augment_labels(lines, p)
            assert np.array_equal(p.boxes_after, d["after"])
            base = crop(cloud, k) if crop is not None else cloud
            moved = R.apply(base, d)
            ref = ov.voxelize(moved, "Car")
            assert np.array_equal(feats[i].cpu().numpy(), ref["feature_buffer"]), (k, d["mode"])
            assert np.array_equal(nums[i].cpu().numpy(), ref["number_buffer"]), (k, d["mode"])
            c = coords[i].cpu().numpy()
            assert np.array_equal(c[:, 1:], ref["coordinate_buffer"]) and (c[:, 0] == i).all()
            # and the augmentation did change what the voxelizer saw (every frame here holds points inside its cars)
            assert (moved != base).any(1).sum() >= 20, (k, d["mode"])
            plain = ov.voxelize(base, "Car")
            assert not (plain["feature_buffer"].shape == ref["feature_buffer"].shape
                        and np.array_equal(plain["feature_buffer"], ref["feature_buffer"])), (k, d["mode"])
            k += 1
    return modes


def test_augmenting_batcher_matches_the_host_replay(tmp_path):
    from voxelnet_amd import dataset as D
    from voxelnet_amd import model as M
    from voxelnet_amd.optim import ClipSGD
    root = str(tmp_path / "kitti")
    _make_kitti(root, 7)
    ds = D.KITTIDataset(root, shuffle=False, augment=False)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=list, num_workers=0)
    np.random.seed(4321)
    batches = list(D.DeviceBatcher(loader, DEV, "Car", augment=True))
    assert [len(b[0]) for b in batches] == [2, 2, 2, 1]
    np.random.seed(4321)
    modes = _check_batches(root, batches)
    print("modes:", modes)
    assert set(modes) == {"boxes", "rotate", "scale"}, modes          # (a property of the seed; checked on the CPU beforehand)
    # one train step on an augmented batch: labels -> device targets -> loss -> backward -> update, one library call
    M.set_precision("bf16")
    torch.manual_seed(0)
    model = M.RPN3D("Car").to(DEV).train(True)
    opt = ClipSGD(list(model.parameters()), 0.01, 5.0)
    assert model._step_fused_ok("bf16", opt)
    out = model.train_step(batches[0], DEV, opt)
    torch.cuda.synchronize()
    assert torch.isfinite(out[2]).item()
    # and through autograd
    out = model(batches[1], DEV)
    out[2].backward()
    assert torch.isfinite(out[2]).item() and all(p.grad is not None for p in model.parameters())


def test_augmenting_batcher_behind_the_fov_crop(tmp_path, golden):
    """copy -> field-of-view crop (padded, NaN tail) -> augment -> voxelize, against crop -> restatement -> oracle"""
    from voxelnet_amd import dataset as D
    from voxelnet_amd.fov import load_calib
    g = golden("fov_crop")
    rows, cols = (int(v) for v in g["image_shape"])
    root = str(tmp_path / "kitti")
    _make_kitti(root, 4, calib=g)
    ds = D.KITTIDataset(root, shuffle=False, load_images=False)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=list, num_workers=0)

    def crop(cloud, k):
        P, Tr, Rr = load_calib(os.path.join(root, "calib", f"{k:06d}.txt"))
        kept, _ = of.fov_crop(cloud, P, Tr, Rr, rows, cols)
        assert 0 < kept.shape[0] < cloud.shape[0]
        return kept
    np.random.seed(99)
    batches = list(D.DeviceBatcher(loader, DEV, "Car", fov_calib_dir=os.path.join(root, "calib"), image_shape=(rows, cols), augment=True))
    np.random.seed(99)
    modes = _check_batches(root, batches, crop)
    print("modes:", modes)
    assert set(modes) == {"boxes", "rotate", "scale"}, modes


def test_augment_false_is_the_pipeline_as_it_was(tmp_path, monkeypatch):
    """augment=False equals omitting the argument bit for bit: same np.random consumption, same outputs, and the new
    entry point is never called"""
    from voxelnet_amd import _lib
    from voxelnet_amd import dataset as D
    root = str(tmp_path / "kitti")
    _make_kitti(root, 3)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    runs = []
    for kw in ({}, {"augment": False}):
        ds = D.KITTIDataset(root, shuffle=False, augment=False)
        loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=list, num_workers=0)
        np.random.seed(7)
        batches = list(D.DeviceBatcher(loader, DEV, "Car", **kw))
        runs.append((batches, np.random.random()))
    assert "vn_augment_points" not in calls and "vn_voxelize_index" in calls
    (a, ta), (b, tb) = runs
    assert ta == tb
    for x, y in zip(a, b):
        assert x[0] == y[0] and all(list(p) == list(q) for p, q in zip(x[1], y[1]))
        for j in (2, 3, 4):
            assert all(torch.equal(p, q) for p, q in zip(x[j], y[j]))
        assert all(np.array_equal(p, q) for p, q in zip(x[6], y[6]))
    # the labels are the files' lines, untouched
    assert list(a[0][1][0]) == open(os.path.join(root, "label_2", "000000.txt")).readlines()
    # with the switch on, the same loader does call it
    ds = D.KITTIDataset(root, shuffle=False, augment=False)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=list, num_workers=0)
    list(D.DeviceBatcher(loader, DEV, "Car", augment=True))
    assert "vn_augment_points" in calls
