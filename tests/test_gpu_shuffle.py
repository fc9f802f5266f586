"""GPU: the device half of the point shuffle — `vn_permute_points` and `vn_shuffle_points` (csrc/shuffle.hip through
voxelnet_amd.shuffle) against tests/shuffle_ref.py, BIT-EQUAL as int32 views (a row is moved, never computed on), and the
`shuffle_points="index" | "device"` switch of DeviceCollate / DeviceBatcher: "index" against `True` under the same seed
(voxel buffers, labels and the np.random state bit for bit), "device" against a host replay (the restatement's
permutation, then the oracle voxelizer)."""
import functools
import os

import numpy as np
import pytest
import torch

import augment_ref as AR
import gtsample_ref as GR
import shuffle_ref as R
from oracle import voxelize as ov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = np.array([1, 2, 3, 4, 5, 6], dtype=np.uint32)
SENTINEL = 0x5A5A5A5A
TAIL = 8                    # sentinel rows behind out[n]


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _cloud(n, seed):
    """(n,4) float32 with rows no arithmetic would carry through: NaNs with distinct payloads (quiet, signalling, negative),
    -0.0 and +-inf, every one of them in each column somewhere"""
    rng = np.random.default_rng(seed)
    bits = rng.standard_normal((n, 4)).astype(np.float32).view(np.uint32).copy()
    special = [0x7FC00000, 0x7FC00001, 0x7FC12345, 0xFFC00007, 0x7F800001, 0xFFBFFFFF, 0x80000000, 0x7F800000, 0xFF800000]
    for j, word in enumerate(special):
        if n:
            bits[(j * 29) % n, j % 4] = word
    if n > 40:
        bits[37] = [0x7FC00100, 0x7FC00200, 0x7FC00300, 0x7FC00400]          # a whole NaN row, four payloads
        bits[38] = [0x80000000] * 4
    return bits.view(np.float32)


def _run(kind, cloud, arg):
    """one call into a buffer with TAIL sentinel rows behind it -> (out rows as int32, tail as uint32)"""
    from voxelnet_amd import shuffle as S
    n = cloud.shape[0]
    pts = torch.from_numpy(cloud.copy()).to(DEV)
    big = torch.full((n + TAIL, 4), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    out = big[:n]
    fn = S.permute_points_device if kind == "permute" else S.shuffle_points_device
    got = fn(pts, arg, out=out)
    assert got is out
    torch.cuda.synchronize()
    assert np.array_equal(pts.cpu().numpy().view(np.int32), cloud.view(np.int32))          # the input is only read
    host = big.cpu().numpy().view(np.uint32)
    return host[:n].view(np.int32), host[n:]


@pytest.mark.parametrize("n", [0, 1, 2, 3, 255, 256, 257, 1023, 1025, 4097, 20000, 311000])
def test_kernels_are_bit_equal_to_the_restatement(n):
    cloud = _cloud(n, 100 + n)
    index = np.random.default_rng(n).permutation(n).astype(np.int32)
    keys = np.random.RandomState(n).randint(0, 2 ** 32, 6, dtype=np.uint32)
    want_perm = R.permute_points(cloud, index).view(np.int32)
    for kind, arg, want in (("permute", index, want_perm), ("shuffle", KEYS, R.shuffle_points(cloud, KEYS).view(np.int32)),
                            ("shuffle", keys, R.shuffle_points(cloud, keys).view(np.int32))):
        first, tail = _run(kind, cloud, arg)
        assert first.shape == (n, 4) and np.array_equal(first, want), (kind, n)
        assert (tail == SENTINEL).all(), (kind, n)                         # nothing behind out[n] is written
        again, _ = _run(kind, cloud, arg)
        assert np.array_equal(again, first), (kind, n)                      # two runs, the same bits
    if n > 3:
        assert not np.array_equal(want_perm, cloud.view(np.int32))
    # without `out`: a new tensor, the same rows; an index table that is on the device already is taken as it is
    from voxelnet_amd import shuffle as S
    pts = torch.from_numpy(cloud.copy()).to(DEV)
    assert np.array_equal(S.shuffle_points_device(pts, KEYS).cpu().numpy().view(np.int32), R.shuffle_points(cloud, KEYS).view(np.int32))
    assert np.array_equal(S.permute_points_device(pts, torch.from_numpy(index).to(DEV)).cpu().numpy().view(np.int32), want_perm)


def test_an_index_outside_the_cloud_gives_a_nan_row_and_reads_nothing():
    n = 257
    cloud = _cloud(n, 7)
    index = np.random.default_rng(3).permutation(n).astype(np.int64)
    bad = {0: -1, 5: n, 100: 2 ** 31 - 1, 255: -2 ** 31, 256: n + 1, 64: -n}
    for row, v in bad.items():
        index[row] = v
    index[9] = index[10]                                                    # and a table need not be a permutation
    got, tail = _run("permute", cloud, index.astype(np.int32))
    want = R.permute_points(cloud, index).view(np.int32)
    assert np.array_equal(got, want) and (tail == SENTINEL).all()
    assert (got[sorted(bad)] == 0x7FC00000).all()
    ok = np.setdiff1d(np.arange(n), sorted(bad))
    assert np.array_equal(got[ok], cloud.view(np.int32)[index[ok]])


def test_on_a_side_stream_and_what_the_wrappers_refuse():
    from voxelnet_amd import _lib
    from voxelnet_amd import shuffle as S
    cloud = _cloud(5000, 11)
    index = np.random.default_rng(5).permutation(5000).astype(np.int32)
    side = torch.cuda.Stream(DEV)
    pts = torch.from_numpy(cloud).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        a, keep_a = S.enqueue_permute_points(pts, index)
        b, keep_b = S.enqueue_shuffle_points(a, KEYS)
    side.synchronize()
    assert any(t.is_pinned() for t in keep_a if torch.is_tensor(t) and not t.is_cuda)          # staged through pinned memory
    assert any(isinstance(t, np.ndarray) and t.dtype == np.uint32 for t in keep_b)
    assert np.array_equal(b.cpu().numpy().view(np.int32), R.shuffle_points(R.permute_points(cloud, index), KEYS).view(np.int32))
    with pytest.raises(_lib.VoxelnetHipError):                              # a gather cannot run in place
        S.permute_points_device(pts, index, out=pts)
    with pytest.raises(_lib.VoxelnetHipError):
        S.shuffle_points_device(pts, KEYS, out=pts)
    with pytest.raises(ValueError):
        S.permute_points_device(pts, index[:-1])
    with pytest.raises(ValueError):
        S.shuffle_points_device(pts, KEYS[:5])
    with pytest.raises(_lib.VoxelnetHipError):
        S.permute_points_device(pts[:, :3], index)


# ---------------------------------------------------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------------------------------------------------
def _make_kitti(root, n, calib=None):
    """a throw-away KITTI directory as tests/test_gpu_dataset._make_kitti; with `calib`, raw sweeps (points all round the
    car) and the calibration files, as tests/test_gpu_augment._make_kitti"""
    from voxelnet_amd import synth
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "targets_car.npz"))
    for d in ("image_2", "velodyne", "label_2") + (("calib",) if calib is not None else ()):
        os.makedirs(os.path.join(root, d))
    for i in range(n):
        tag = f"{i:06d}"
        cloud = synth.synth_cloud("Car", 800 + 100 * i, 500 + i, 2.3, 35)
        if calib is not None:
            rng = np.random.default_rng(40 + i)
            extra = np.stack([rng.uniform(-70, 70, 3000), rng.uniform(-40, 40, 3000), rng.uniform(-3, 1, 3000),
                              np.round(rng.uniform(0, 1, 3000), 2)], 1).astype(np.float32)
            cloud = np.concatenate([cloud, extra])[rng.permutation(len(cloud) + 3000)]
            with open(os.path.join(root, "calib", tag + ".txt"), "w") as fh:
                def fmt(name, a):
                    return name + ": " + " ".join(f"{v:.12e}" for v in np.asarray(a).reshape(-1))
                fh.write("\n".join([fmt("P0", calib["P"]), fmt("P1", calib["P"]), fmt("P2", calib["P"]), fmt("P3", calib["P"]),
                                    fmt("R0_rect", calib["R"][:3, :3]), fmt("Tr_velo_to_cam", calib["Tr"][:3]),
                                    fmt("Tr_imu_to_velo", calib["Tr"][:3])]) + "\n")
        np.ascontiguousarray(cloud, dtype=np.float32).tofile(os.path.join(root, "velodyne", tag + ".bin"))
        with open(os.path.join(root, "label_2", tag + ".txt"), "w") as f:
            f.write("\n".join(str(s) for s in g[f"labels{i % 4}"]) + "\n")
        # (no images: load_images=False)
        open(os.path.join(root, "image_2", tag + ".png"), "wb").close()


def _read(root, k):
    cloud = np.fromfile(os.path.join(root, "velodyne", f"{k:06d}.bin"), dtype=np.float32).reshape(-1, 4)
    return cloud, open(os.path.join(root, "label_2", f"{k:06d}.txt")).readlines()


def _batches(root, seed, **kw):
    from voxelnet_amd import dataset as D
    ds = D.KITTIDataset(root, shuffle=False, augment=False, load_images=False)
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=list, num_workers=0)
    np.random.seed(seed)
    batches = list(D.DeviceBatcher(loader, DEV, "Car", **kw))
    torch.cuda.synchronize()
    return batches, np.random.get_state()


@functools.lru_cache(maxsize=None)
def _sampler_entries():
    """a small database by the restatement (frames 8..11: 24 cars), computed once and left unchanged"""
    from voxelnet_amd import synth
    return tuple(GR.database([(f"{f + 100:06d}", synth.synth_cloud("Car", 6000, synth.frame_seed(2, f), 2.3, 35),
                               synth.synth_labels("Car", 6, f)) for f in range(8, 12)]))


def _sampler():
    from voxelnet_amd import gtsample as G
    db = G.GTDatabase([G.GTEntry(e["cls"], e["tag"], e["box"].copy(), e["points"].copy(), e["line"]) for e in _sampler_entries()])
    return G.GTSampler(db, per_class={"Car": 15}, min_points=5)


@pytest.mark.parametrize("config", ["plain", "fov", "augment+paste"])
def test_index_mode_is_the_host_shuffle_bit_for_bit(tmp_path, golden, monkeypatch, config):
    """shuffle_points="index" against True under the same seed: feature, number and coordinate buffers, labels and the
    np.random state after the batches"""
    from voxelnet_amd import _lib
    g = golden("fov_crop")
    root = str(tmp_path / "kitti")
    _make_kitti(root, 2, calib=g if config == "fov" else None)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    kw = {}
    if config == "fov":
        kw = dict(fov_calib_dir=os.path.join(root, "calib"), image_shape=tuple(int(v) for v in g["image_shape"]))
    runs = {}
    for mode in (True, "index"):
        if config == "augment+paste":
            kw = dict(augment=True, gt_sampler=_sampler())
        del calls[:]
        runs[mode] = _batches(root, 4242, shuffle_points=mode, **kw) + (list(calls),)
    (a, state_a, calls_a), (b, state_b, calls_b) = runs[True], runs["index"]
    assert _same_state(state_a, state_b)
    assert "vn_permute_points" not in calls_a and calls_b.count("vn_permute_points") == 2 and "vn_shuffle_points" not in calls_b
    assert [c for c in calls_b if c != "vn_permute_points"] == calls_a          # and nothing else changes
    if config == "fov":
        assert calls_a.count("vn_fov_crop") == 2
    if config == "augment+paste":
        assert calls_a.count("vn_augment_points") == 2 and calls_a.count("vn_gt_paste") >= 1
    assert len(a) == len(b) == 1
    for x, y in zip(a, b):
        assert x[0] == y[0] and all(list(p) == list(q) for p, q in zip(x[1], y[1]))
        for j in (2, 3, 4):
            assert len(x[j]) == len(y[j]) == 2 and all(torch.equal(p, q) for p, q in zip(x[j], y[j]))
            assert all(p.shape[0] > 100 for p in x[j])
        for i in range(2):
            cloud, _ = _read(root, i)
            assert np.array_equal(y[6][i], cloud)                            # "index": element 6 is the cloud as read
            assert not np.array_equal(x[6][i], cloud) and np.array_equal(np.sort(x[6][i], 0), np.sort(cloud, 0))


@pytest.mark.parametrize("augment", [False, True])
def test_device_mode_matches_the_host_replay(tmp_path, augment):
    """shuffle_points="device": keys drawn where the host shuffle stood (the sample's first draw), the restatement's
    permutation of the cloud as read, [the augmentation's restatement], the oracle voxelizer"""
    from voxelnet_amd import augment as A
    root = str(tmp_path / "kitti")
    _make_kitti(root, 2)
    batches, state = _batches(root, 777, shuffle_points="device", augment=augment)
    assert len(batches) == 1
    tags, label, feats, nums, coords, rgb, raw = batches[0]
    np.random.seed(777)
    for i in range(2):
        cloud, lines = _read(root, i)
        keys = np.random.randint(0, 2 ** 32, 6, dtype=np.uint32)
        shuffled = R.shuffle_points(cloud, keys)
        assert not np.array_equal(shuffled, cloud)
        if augment:
            before = np.random.get_state()
            d = AR.draw(lines)
            np.random.set_state(before)
            assert list(label[i]) == A.augment_labels(lines, A.draw_augmentation(lines))
            shuffled = AR.apply(shuffled, d)
        else:
            assert list(label[i]) == lines
        assert np.array_equal(raw[i], cloud)                                 # element 6 is the cloud as read
        ref = ov.voxelize(shuffled, "Car")
        assert np.array_equal(feats[i].cpu().numpy(), ref["feature_buffer"]), i
        assert np.array_equal(nums[i].cpu().numpy(), ref["number_buffer"]), i
        c = coords[i].cpu().numpy()
        assert np.array_equal(c[:, 1:], ref["coordinate_buffer"]) and (c[:, 0] == i).all()
        # and the order did decide something: the cloud as read fills its crowded voxels with other points
        assert not np.array_equal(ov.voxelize(cloud, "Car")["feature_buffer"], ref["feature_buffer"])
    assert _same_state(np.random.get_state(), state)


@pytest.mark.parametrize("mode", ["index", "device"])
def test_the_callers_arrays_are_left_alone(tmp_path, mode):
    from voxelnet_amd import dataset as D
    root = str(tmp_path / "kitti")
    _make_kitti(root, 2)
    ds = D.KITTIDataset(root, shuffle=False, load_images=False)
    parts = [ds[0], ds[1]]
    as_read = [p[2].copy() for p in parts]
    np.random.seed(3)
    batch = D.DeviceCollate(DEV, "Car", shuffle_points=mode)(parts)
    torch.cuda.synchronize()
    for i in range(2):
        assert np.array_equal(parts[i][2], as_read[i]) and batch[6][i] is parts[i][2]
        assert np.array_equal(as_read[i], _read(root, i)[0])


def test_the_host_shuffle_is_the_pipeline_as_it_was(tmp_path, monkeypatch):
    """shuffle_points=True, "host" and the default: nothing new is launched, the caller's array is shuffled in place, the
    buffers are the oracle's on a replay of np.random.shuffle; False: no draw at all"""
    from voxelnet_amd import _lib
    from voxelnet_amd import dataset as D
    root = str(tmp_path / "kitti")
    _make_kitti(root, 2)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    runs = [_batches(root, 99, **kw) for kw in ({}, {"shuffle_points": True}, {"shuffle_points": "host"})]
    assert "vn_permute_points" not in calls and "vn_shuffle_points" not in calls and "vn_voxelize_index" in calls
    np.random.seed(99)
    refs = []
    for i in range(2):
        cloud, _ = _read(root, i)
        np.random.shuffle(cloud)
        refs.append((cloud, ov.voxelize(cloud, "Car")))
    today = np.random.get_state()
    for batches, state in runs:
        assert _same_state(state, today) and len(batches) == 1
        tags, label, feats, nums, coords, rgb, raw = batches[0]
        for i, (cloud, ref) in enumerate(refs):
            assert np.array_equal(raw[i], cloud) and list(label[i]) == _read(root, i)[1]
            assert np.array_equal(feats[i].cpu().numpy(), ref["feature_buffer"])
            assert np.array_equal(nums[i].cpu().numpy(), ref["number_buffer"])
            assert np.array_equal(coords[i].cpu().numpy()[:, 1:], ref["coordinate_buffer"])
    np.random.seed(99)
    before = np.random.get_state()
    ds = D.KITTIDataset(root, shuffle=False, load_images=False)
    batch = D.DeviceCollate(DEV, "Car", shuffle_points=False)([ds[0], ds[1]])
    assert _same_state(np.random.get_state(), before)
    for i in range(2):
        assert np.array_equal(batch[6][i], _read(root, i)[0])
        assert np.array_equal(batch[2][i].cpu().numpy(), ov.voxelize(_read(root, i)[0], "Car")["feature_buffer"])
