"""CPU: the directed clouds of tests/voxel_cases.py.

(1) On every cloud the C oracle (oracle/voxelize_ref.c), its numpy twin (the reference's own expressions, utils.py:37-88)
    and the library's host entry (csrc/voxelize_host.hip) agree bit for bit: int64 coordinates and counts, fp32 feature
    BITS (uint32 views: -0.0 is not +0.0, and a NaN intensity compares equal to itself).
(2) Every cloud contains what it was built for — asserted ON THE REFERENCE ALONE, so that the GPU tests that import the
    same builders compare the device on inputs that do have teeth.  A cloud that stops holding a condition fails here;
    the remedy is a wider neighbour range or another seed, never a weaker condition.

Counts measured with +-2 ulp neighbours (points of the axis / key differs under reciprocal-multiply / under a float64
add-divide-floor chain): Car x 1765 / 91 / 187, Car y 2005 / 157 / 488, Pedestrian x 1205 / 56 / 118, Pedestrian y
1005 / 78 / 241, z (both grids) 55 / 0 / 12."""
import numpy as np
import pytest

import voxel_cases as V
from oracle import voxelize as ov

CASE_IDS = [c.id for c in V.all_cases()]
KEYS = ("feature_buffer", "coordinate_buffer", "number_buffer")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_buffers(got, ref, what):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
    assert np.array_equal(got["coordinate_buffer"], ref["coordinate_buffer"]), what
    assert np.array_equal(got["number_buffer"], ref["number_buffer"]), what
    assert np.array_equal(bits(got["feature_buffer"]), bits(ref["feature_buffer"])), what


def kept_rows(ref):
    """the (x, y, z, intensity) bits of every point the reference kept, as a set of 4-tuples"""
    f, n = ref["feature_buffer"], ref["number_buffer"]
    real = np.arange(f.shape[1])[None, :] < n[:, None]
    return {tuple(r) for r in bits(f[:, :, :4])[real].tolist()}


def has_rows(rows, pts):
    return [tuple(r) in rows for r in bits(pts).tolist()]


# ------------------------------------------------------------------------------------------ three implementations
@pytest.mark.parametrize("case_id", CASE_IDS)
def test_oracle_numpy_twin_and_host_entry_agree_bit_for_bit(case_id):
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.voxelize import voxelize_host
    c = V.case(case_id)
    ref = V.reference(case_id)
    g = V.grid(c.target, c.overrides)
    K = ref["number_buffer"].shape[0]
    assert ref["feature_buffer"].shape == (K, g["T"], 7) and ref["feature_buffer"].dtype == np.float32
    assert ref["coordinate_buffer"].shape == (K, 3) and ref["coordinate_buffer"].dtype == np.int64
    assert ref["number_buffer"].dtype == np.int64
    with np.errstate(all="ignore"):
        twin = ov.voxelize_numpy(c.points, c.target, **c.overrides)
        f, co, n = voxelize_host(c.points, grid_config(c.target, **c.overrides), 0, coord_cols=3)
    assert_same_buffers(twin, ref, "numpy twin vs C oracle")
    assert_same_buffers({"feature_buffer": f, "coordinate_buffer": co, "number_buffer": n}, ref, "host entry vs C oracle")


@pytest.mark.parametrize("case_id", ["boundary-Pedestrian", "grid2x5x7-full"])
def test_host_entry_batch_column(case_id):
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.voxelize import voxelize_host
    c, ref = V.case(case_id), V.reference(case_id)
    f, co, n = voxelize_host(c.points, grid_config(c.target, **c.overrides), 5, coord_cols=4)
    assert co.shape == (len(n), 4) and (co[:, 0] == 5).all() and np.array_equal(co[:, 1:], ref["coordinate_buffer"])
    assert np.array_equal(bits(f), bits(ref["feature_buffer"])) and np.array_equal(n, ref["number_buffer"])


# -------------------------------------------------------------------------------------------------- boundary teeth
@pytest.mark.parametrize("target", ["Car", "Pedestrian"])
def test_boundary_cloud_is_its_axis_parts(target):
    pts, tgt, over = V.boundary_cloud(target)
    g = V.grid(target, {})
    parts = np.concatenate([V.boundary_axis_points(target, a) for a in "xyz"])
    assert tgt == target and over == {} and pts.dtype == np.float32
    assert pts.shape == parts.shape == (5 * (g["W"] + g["H"] + g["D"] + 3), 4)
    order = lambda a: a[np.lexsort(bits(a).T)]                                                    # noqa: E731
    assert np.array_equal(bits(order(pts)), bits(order(parts))) and not np.array_equal(bits(pts), bits(parts))
    # the points spread over many voxels, and both range limits of every axis are probed from both sides
    assert V.reference(f"boundary-{target}")["number_buffer"].shape[0] > len(pts) // 2
    for a in "xyz":
        idx = V.axis_index(V.boundary_axis_points(target, a), g, a)
        n = g[V.AXES[a][0]]
        assert {-1.0, 0.0, n - 1.0, float(n)} <= set(idx.tolist())


@pytest.mark.parametrize("target", ["Car", "Pedestrian"])
@pytest.mark.parametrize("axis", ["x", "y", "z"])
def test_boundary_cloud_tells_the_ieee_divide_from_its_imitations(target, axis):
    g = V.grid(target, {})
    p = V.boundary_axis_points(target, axis)
    n = g[V.AXES[axis][0]]
    ref = V.axis_index(p, g, axis)
    in_range = (ref >= 0) & (ref < n)
    recip = int(((V.axis_index(p, g, axis, "recip") != ref) & in_range).sum())
    f64 = int((V.axis_index(p, g, axis, "f64") != ref).sum())
    print(f"{target} {axis}: {len(p)} points, reciprocal-multiply differs on {recip}, float64 chain on {f64}")
    if axis == "z":
        assert f64 >= 5
    else:
        assert recip >= 50 and f64 >= 50


# --------------------------------------------------------------------------------------------------- segment teeth
@pytest.mark.parametrize("T", V.SEGMENT_T)
def test_segment_cloud_holds_its_conditions(T):
    pts, target, over = V.segment_cloud(T)
    assert over == {"T": T}
    g = V.grid(target, over)
    ref = V.reference(f"segment-T{T}")
    n = ref["number_buffer"]
    assert (n == T).any() and n.max() == T
    if T > 1:
        assert (n < T).any()
    key = V.linear_key(pts, g)
    assert (key >= 0).all()
    per_voxel = np.bincount(np.unique(key, return_inverse=True)[1])
    print(f"T={T}: {len(pts)} points, {len(per_voxel)} voxels, input points per hot voxel {sorted(per_voxel[per_voxel > 1].tolist())}")
    assert set(V.segment_sizes(T)) <= set(per_voxel.tolist())
    assert (per_voxel > 64).any() and (per_voxel == 64).any() and {63, 65, 127, 128, 129, 700} <= set(per_voxel.tolist())
    # exact duplicates are present, inside a voxel that overflows T
    uniq, cnt = np.unique(bits(pts), axis=0, return_counts=True)
    assert (cnt > 1).sum() >= 5
    # "first T in input order" is not "T smallest by x": the same points, sorted by x, give other features
    by_x = ov.voxelize(pts[np.argsort(pts[:, 0], kind="stable")], target, **over)
    assert np.array_equal(by_x["coordinate_buffer"], ref["coordinate_buffer"]) and np.array_equal(by_x["number_buffer"], n)
    assert not np.array_equal(bits(by_x["feature_buffer"][:, :, :4]), bits(ref["feature_buffer"][:, :, :4]))
    # nor is a voxel's input order an ascending order of any column
    hot = pts[key == np.unique(key)[np.argmax(per_voxel)]]
    assert all((np.diff(hot[:, col]) < 0).any() for col in range(4))


# -------------------------------------------------------------------------------------------------- tile-seam teeth
def test_tile_seam_cloud_holds_its_conditions():
    pts, target, over = V.tile_seam_cloud()
    g = V.grid(target, over)
    cells = g["D"] * g["H"] * g["W"]
    want = V.tile_seam_cells()
    ref = V.reference("tile-seam")
    c = ref["coordinate_buffer"]
    assert ref["number_buffer"].shape[0] == len(want) == 14 + 2 * V.SCAN_TILE
    assert np.array_equal((c[:, 0] * g["H"] + c[:, 1]) * g["W"] + c[:, 2], want)
    assert np.array_equal(np.unique(V.linear_key(pts, g)), want)
    assert set(ref["number_buffer"].tolist()) == {1, 2}
    listed = {0, 7, 8, 2047, 2048, 2049, 2048 * 255 - 1, 2048 * 255 + 1, 2048 * 256 - 1, 2048 * 256 + 1, 2048 * 512 - 1,
              2048 * 512 + 1, cells - 2, cells - 1}
    assert listed <= set(want.tolist())
    tiles = want // V.SCAN_TILE
    full = np.flatnonzero(np.bincount(tiles) == V.SCAN_TILE)
    assert len(full) == 1                                                      # the run that starts at a tile boundary
    part = np.bincount(tiles)[[400, 401]]
    assert part.sum() == V.SCAN_TILE and (part > 0).all()                      # the run that straddles one
    assert cells > 2 * V.SCAN_WIDTH * V.SCAN_TILE and cells % V.SCAN_TILE != 0  # third trip of k_scan_blocks; partial last tile


# -------------------------------------------------------------------------------------------------- small grids
def test_small_grid_clouds_hold_their_conditions():
    cases = V.small_grid_clouds()
    assert [c.id.split("-")[0] for c in cases[::2]] == [f"grid{d}x{h}x{w}" for d, h, w in V.SMALL_GRIDS]
    assert [d * h * w for d, h, w in V.SMALL_GRIDS] == [15, V.SCAN_TILE, V.SCAN_TILE + 1, 70]
    for c in cases:
        g = V.grid(c.target, c.overrides)
        cells = g["D"] * g["H"] * g["W"]
        n = V.reference(c.id)["number_buffer"]
        if c.id.endswith("full"):
            assert len(n) == cells < len(c.points) and set(n.tolist()) == {1, 2, 3}
        else:
            assert len(n) == len(c.points) == (cells + 1) // 2 and (n == 1).all()


# --------------------------------------------------------------------------------------------- counts, slot reuse
def test_count_clouds_hold_their_conditions():
    cases = V.count_clouds()
    assert [len(c.points) for c in cases] == [n for n in V.COUNTS for _ in range(2)]
    for c in cases:
        ref = V.reference(c.id)
        K = 0 if c.id.endswith("outside") else len(c.points)
        assert ref["number_buffer"].shape == (K,) and (ref["number_buffer"] == 1).all()
        assert ref["coordinate_buffer"].shape == (K, 3) and ref["feature_buffer"].shape == (K, 35, 7)


def test_slot_reuse_clouds_hold_their_conditions():
    large, small, none = V.slot_reuse_clouds()
    assert len(large.points) == len(small.points) == len(none.points) == V.SLOT_N
    K = [V.reference(c.id)["number_buffer"].shape[0] for c in (large, small, none)]
    print("slot reuse K:", K)
    assert K[0] > V.SLOT_N // 2 and 0 < K[1] < 10 and K[2] == 0
    assert V.reference(small.id)["number_buffer"].max() == 35


# ------------------------------------------------------------------------------------------------ non-finite teeth
def test_nonfinite_cloud_holds_its_conditions():
    pts, target, over = V.nonfinite_cloud()
    parts = V.nonfinite_parts()
    assert target == "Car" and over == {} and len(pts) == sum(len(p) for p in parts.values())
    ref = V.reference("nonfinite")
    rows = kept_rows(ref)
    bad = parts["bad_coordinate"]
    assert len(bad) == 15 and np.isnan(bad).sum() == 3 and np.isinf(bad).sum() == 6 and (np.abs(bad[:, :3]) == np.float32(1e30)).sum() == 6
    assert not any(has_rows(rows, bad))
    sub = np.float32(2.0 ** -149)
    nz, ns, ps = parts["neg_zero_x"], parts["neg_subnormal_x"], parts["pos_subnormal_x"]
    assert np.signbit(nz[0, 0]) and nz[0, 0] == 0 and ns[0, 0] == -sub and ps[0, 0] == sub and sub > 0
    assert all(has_rows(rows, nz)) and all(has_rows(rows, ps)) and not any(has_rows(rows, ns))
    co = ref["coordinate_buffer"]
    assert ((co[:, 2] == 0) & (co[:, 0] == 6)).sum() == 2                      # their two voxels: cell x = 0
    assert all(has_rows(rows, parts["odd_intensity"])) and all(has_rows(rows, parts["ordinary"]))
    f = ref["feature_buffer"]
    assert np.isnan(f[:, :, 3]).sum() == 1 and np.isinf(f[:, :, 3]).sum() == 2 and not np.isnan(f[:, :, [0, 1, 2, 4, 5, 6]]).any()
    # two voxels whose kept points have a negative zero in a coordinate; in the first the offset from the centroid is -0 too
    nzv = parts["neg_zero_voxels"]
    assert all(has_rows(rows, nzv))
    real = np.arange(f.shape[1])[None, :] < ref["number_buffer"][:, None]
    neg_zero = (bits(f) == 0x80000000) & real[:, :, None]
    assert neg_zero[:, :, 1].any(1).sum() == 1 and neg_zero[:, :, 2].any(1).sum() == 1
    assert neg_zero[:, :, 1].sum() == 3 and neg_zero[:, :, 5].sum() == 3 and neg_zero[:, :, 2].sum() == 2
    # which np.array_equal on floats could not see
    flipped = f.copy()
    flipped.view(np.uint32)[neg_zero] = 0
    assert np.array_equal(flipped[:, :, :3], f[:, :, :3]) and not np.array_equal(bits(flipped), bits(f))
    assert not np.array_equal(f, f)                                             # (NaN intensity)
