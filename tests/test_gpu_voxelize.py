"""GPU: HIP voxelizer + scatter through the C ABI vs the oracle and the golden
vectors of the imported reference (utils.py:10-100, model.py:102-106).
Bar: coordinates/counts bit-exact (int64), features bit-exact (fp32 bits: every feature comparison is on uint32 views).

The directed clouds of tests/voxel_cases.py (tests/test_voxel_cases_host.py asserts on the reference alone what each of
them contains) go through voxelize_device, through voxelize_device_async with and without a VoxelBuffers slot, and
through one reused slot whose rows past K must stay untouched."""
import hashlib

import numpy as np
import pytest
import torch

import voxel_cases as V

pytestmark = pytest.mark.gpu

CASE_IDS = [c.id for c in V.all_cases()]
ASYNC_IDS = [i for i in CASE_IDS if i.startswith(("boundary", "segment", "tile-seam")) or i.endswith("outside")]
FEATURE_SENTINEL = 0x7FC0BAD1          # a quiet-NaN bit pattern (as int32) that no input carries
INT_SENTINEL = -7


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_buffers_bit_equal(out, ref):
    """dtypes, shapes, int64 coordinates and counts, fp32 feature BITS (-0.0 is not +0.0; a NaN equals itself)"""
    for k in ("feature_buffer", "coordinate_buffer", "number_buffer"):
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, (k, out[k].shape, ref[k].shape)
    assert np.array_equal(out["coordinate_buffer"], ref["coordinate_buffer"])
    assert np.array_equal(out["number_buffer"], ref["number_buffer"])
    assert np.array_equal(bits(out["feature_buffer"]), bits(ref["feature_buffer"]))


def hip_voxelize(points, target, T=None, batch_index=0, coord_cols=3, **kw):
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.voxelize import voxelize_device
    g = grid_config(target, T=T, **kw)
    f, c, n = voxelize_device(torch.from_numpy(np.array(points)).cuda(), g, batch_index, coord_cols=coord_cols)
    return {"feature_buffer": f.cpu().numpy(), "coordinate_buffer": c.cpu().numpy(), "number_buffer": n.cpu().numpy()}


@pytest.mark.parametrize("tag,target", [("car", "Car"), ("ped", "Pedestrian")])
def test_golden_small_bit_exact(golden, tag, target):
    g = golden(f"voxelize_{tag}_small")
    out = hip_voxelize(g["points"], target)
    assert np.array_equal(out["coordinate_buffer"], g["coordinate_buffer"])
    assert np.array_equal(out["number_buffer"], g["number_buffer"])
    assert np.array_equal(out["feature_buffer"].view(np.uint32), g["feature_buffer"].view(np.uint32))


def test_degenerate(golden):
    g = golden("voxelize_degenerate")
    out = hip_voxelize(g["far_points"], "Car")
    assert out["coordinate_buffer"].shape == (0, 3) and out["feature_buffer"].shape == (0, 35, 7)
    one = hip_voxelize(g["one_points"], "Car")
    assert one["feature_buffer"].dtype == np.float32 and g["one_feature"].dtype == np.float32
    assert np.array_equal(bits(one["feature_buffer"]), bits(g["one_feature"]))
    assert np.array_equal(one["coordinate_buffer"], g["one_coord"])
    empty = hip_voxelize(np.zeros((0, 4), np.float32), "Car")
    assert empty["number_buffer"].shape == (0,)


@pytest.mark.parametrize("cfg_id,target", [(2, "Car"), (3, "Pedestrian")])
def test_full_size_digest(golden, cfg_id, target):
    from voxelnet_amd import synth
    g = golden("voxelize_full_digest")
    w = synth.WORKLOADS[cfg_id]
    cloud = synth.synth_cloud(target, w["k0"], synth.frame_seed(cfg_id, 0), w["mean_extra"], w["T"])
    np.random.seed(7)
    np.random.shuffle(cloud)
    out = hip_voxelize(cloud, target)
    assert out["coordinate_buffer"].shape[0] == int(g[f"cfg{cfg_id}_K"])
    assert sha(out["coordinate_buffer"]) == str(g[f"cfg{cfg_id}_coord_sha"])
    assert sha(out["number_buffer"]) == str(g[f"cfg{cfg_id}_number_sha"])
    assert sha(out["feature_buffer"]) == str(g[f"cfg{cfg_id}_feature_sha"])


def test_pcl_to_voxels_dropin_shuffles_in_place(golden):
    """Same call as the reference: shuffles the caller's array (utils.py:35) and
    returns the dict of numpy buffers; replaying the shuffle through the oracle
    gives identical buffers."""
    from oracle import voxelize as ov
    from voxelnet_amd import synth
    from voxelnet_amd.voxelize import pcl_to_voxels, prepare_voxel
    cloud = synth.synth_cloud("Car", 500, 3)
    twin = cloud.copy()
    np.random.seed(123)
    out = pcl_to_voxels(cloud, "Car")
    np.random.seed(123)
    np.random.shuffle(twin)
    assert np.array_equal(cloud, twin)
    ref = ov.voxelize(twin, "Car")
    assert set(out) == set(ref)
    assert_buffers_bit_equal(out, ref)
    f, n, c = prepare_voxel([out, out])
    assert c[1].shape[1] == 4 and (c[1][:, 0] == 1).all()


def test_dense_config5_vs_oracle():
    """BASELINE config 5 shape: 300k points, 40k voxels, T=64 (one frame)."""
    from oracle import voxelize as ov
    from voxelnet_amd import synth
    w = synth.WORKLOADS[5]
    cloud = synth.synth_cloud("Car", w["k0"], synth.frame_seed(5, 0), w["mean_extra"], w["T"])
    assert cloud.shape[0] > 250000
    ref = ov.voxelize(cloud, "Car", T=64)
    out = hip_voxelize(cloud, "Car", T=64)
    assert ref["coordinate_buffer"].shape[0] == 40000
    assert_buffers_bit_equal(out, ref)


def test_hot_voxel_many_points():
    """>64 points in one voxel exercises the long-segment path; first T in input order."""
    from oracle import voxelize as ov
    rng = np.random.default_rng(0)
    hot = np.concatenate([rng.uniform([10.0, 1.0, -1.0, 0], [10.19, 1.19, -0.61, 1], (1000, 4)),
                          rng.uniform([0, -40, -3, 0], [70, 40, 1, 1], (500, 4))]).astype(np.float32)
    rng.shuffle(hot)
    ref = ov.voxelize(hot, "Car")
    out = hip_voxelize(hot, "Car")
    assert_buffers_bit_equal(out, ref)
    assert ref["number_buffer"].max() == 35


# ------------------------------------------------------------------------------- directed clouds (tests/voxel_cases.py)
@pytest.mark.parametrize("case_id", CASE_IDS)
def test_directed_cloud_vs_oracle(case_id):
    """voxel faces +-2 ulp, non-finite and signed-zero inputs, segments around 64 and T, tile seams, grids of less than /
    exactly / just over one scan tile, full grids, K = 0: bit for bit, shapes and dtypes included"""
    c, ref = V.case(case_id), V.reference(case_id)
    out = hip_voxelize(c.points, c.target, **c.overrides)
    T = V.grid(c.target, c.overrides)["T"]
    assert out["feature_buffer"].shape[1:] == (T, 7) and out["coordinate_buffer"].shape[1:] == (3,)
    assert_buffers_bit_equal(out, ref)


@pytest.mark.parametrize("case_id", ["boundary-Car", "boundary-Pedestrian"] + [c.id for c in V.small_grid_clouds()[::2]])
def test_directed_cloud_batch_column(case_id):
    c, ref = V.case(case_id), V.reference(case_id)
    out = hip_voxelize(c.points, c.target, batch_index=3, coord_cols=4, **c.overrides)
    co = out["coordinate_buffer"]
    assert co.dtype == np.int64 and co.shape == (ref["number_buffer"].shape[0], 4) and (co[:, 0] == 3).all()
    assert_buffers_bit_equal(dict(out, coordinate_buffer=np.ascontiguousarray(co[:, 1:])), ref)


def _tensors_bit_equal(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b)) and \
        torch.equal(a[0].contiguous().view(torch.int32), b[0].contiguous().view(torch.int32))


@pytest.mark.parametrize("with_slot", [False, True], ids=["fresh", "slot"])
@pytest.mark.parametrize("case_id", ASYNC_IDS)
def test_async_path_equals_sync_path(case_id, with_slot):
    """the capacity launch that takes K from device memory (what bench.py and the DeviceBatcher run), with and without a
    VoxelBuffers slot, against the launch that knows K"""
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.voxelize import VoxelBuffers, voxelize_device, voxelize_device_async
    c, ref = V.case(case_id), V.reference(case_id)
    g = grid_config(c.target, **c.overrides)
    pts = torch.from_numpy(np.array(c.points)).cuda()
    sync = voxelize_device(pts, g, 2, coord_cols=4)
    slot = VoxelBuffers(pts.shape[0], g, 4, pts.device) if with_slot else None
    got = voxelize_device_async(pts, g, 2, coord_cols=4, buffers=slot).result()
    assert got[0].shape == (ref["number_buffer"].shape[0], g.T, 7) and got[1].shape[1:] == (4,)
    assert _tensors_bit_equal(got, sync)
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(ref["feature_buffer"]))


def test_slot_reuse_writes_nothing_past_k():
    """one VoxelBuffers slot, three clouds of the same N: large K, small K, K = 0.  The gather is launched at capacity and
    reads K from the device; rows >= K have stale cnt / seg_off entries of the frame before, and must stay untouched."""
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.voxelize import VoxelBuffers, voxelize_device_async
    g = grid_config("Car")
    dev = torch.device("cuda", torch.cuda.current_device())
    slot = VoxelBuffers(V.SLOT_N, g, 3, dev)
    assert slot.cap == V.SLOT_N and slot.feature.shape == (V.SLOT_N, g.T, 7)
    for c in V.slot_reuse_clouds():
        ref = V.reference(c.id)
        K = ref["number_buffer"].shape[0]
        slot.feature.view(torch.int32).fill_(FEATURE_SENTINEL)
        slot.coord.fill_(INT_SENTINEL)
        slot.number.fill_(INT_SENTINEL)
        slot.k_host.fill_(INT_SENTINEL)
        f, co, n = voxelize_device_async(torch.from_numpy(np.array(c.points)).to(dev), g, 0, coord_cols=3, buffers=slot).result()
        assert int(slot.k_host[0]) == K, c.id
        assert f.untyped_storage().data_ptr() == slot.feature.untyped_storage().data_ptr() and f.shape[0] == K
        assert_buffers_bit_equal({"feature_buffer": f.cpu().numpy(), "coordinate_buffer": co.cpu().numpy(),
                                  "number_buffer": n.cpu().numpy()}, ref)
        torch.cuda.synchronize()
        assert bool((slot.feature.view(torch.int32)[K:] == FEATURE_SENTINEL).all()), c.id
        assert bool((slot.coord[K:] == INT_SENTINEL).all()) and bool((slot.number[K:] == INT_SENTINEL).all()), c.id


@pytest.mark.parametrize("T", [35, 64])
def test_segment_cloud_twice_gives_identical_bits(T):
    """k_fill places point indices with atomics; the gather's repeated wave-min restores input order"""
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.voxelize import voxelize_device
    c = V.case(f"segment-T{T}")
    g = grid_config(c.target, **c.overrides)
    pts = torch.from_numpy(np.array(c.points)).cuda()
    a = voxelize_device(pts, g, 0, coord_cols=3)
    b = voxelize_device(pts, g, 0, coord_cols=3)
    assert _tensors_bit_equal(a, b)


def test_scatter_fwd_bwd_vs_oracle():
    from oracle import torch_ref as tr
    from voxelnet_amd import ops
    rng = np.random.default_rng(1)
    B, D, H, W, C = 2, 10, 16, 24, 128
    K = 300
    lin = rng.choice(B * D * H * W, K, replace=False)
    coord = np.stack([lin // (D * H * W), (lin // (H * W)) % D, (lin // W) % H, lin % W], 1).astype(np.int64)
    vw = rng.standard_normal((K, C)).astype(np.float32)
    ref = tr.scatter_dense(torch.from_numpy(vw), torch.from_numpy(coord), (B, D, H, W))
    vw_d = torch.from_numpy(vw).cuda().requires_grad_(True)
    dense = ops.scatter_dense(vw_d, torch.from_numpy(coord).cuda(), (B, D, H, W))
    assert torch.equal(dense.detach().cpu(), ref)           # pure data movement: bit-exact
    up = torch.from_numpy(rng.standard_normal(ref.shape).astype(np.float32))
    dense.backward(up.cuda())
    want = up[coord[:, 0], coord[:, 1], coord[:, 2], coord[:, 3]]
    assert torch.equal(vw_d.grad.cpu(), want)
