"""CPU: the directed occupancy sets of tests/sparse_cases.py hold what they were built for — asserted ON THE ORACLE ALONE
(conv3d of the occupancy with an all-ones kernel), so that tests/test_gpu_sparse_first_layer.py compares the device on
inputs that do have teeth.  A set that stops holding a property fails here; the remedy is another placement or seed,
never a weaker property."""
import numpy as np
import pytest

import sparse_cases as S


@pytest.mark.parametrize("case_id", S.ALL_IDS)
def test_coordinates_are_unique_and_inside_the_grid(case_id):
    c = S.case(case_id)
    co = c.coord
    assert co.dtype == np.int64 and co.ndim == 2 and co.shape[1] == 4
    assert (co >= 0).all() and (co < np.array([c.B, c.D, c.H, c.W])).all()
    lin = ((co[:, 0] * c.D + co[:, 1]) * c.H + co[:, 2]) * c.W + co[:, 3]
    assert len(np.unique(lin)) == len(lin)
    if len(lin) > 2:
        assert (np.diff(lin) < 0).any(), "the voxel order must not be sorted"
    sites, taps = S.oracle(case_id)
    Do, Ho, Wo = S.out_dims(c.D, c.H, c.W)
    assert taps.shape == (c.B, Do, Ho, Wo)
    assert int(taps.sum()) <= 27 * len(co) and len(sites) == int((taps > 0).sum())
    slin = ((sites[:, 0] * Do + sites[:, 1]) * Ho + sites[:, 2]) * Wo + sites[:, 3]
    assert (np.diff(slin) > 0).all()                 # ascending linear order, no site twice
    assert len(sites) <= S.PER_VOXEL * len(co)


def test_full_block_has_sites_with_all_27_taps_and_an_odd_depth():
    c = S.case("full_block")
    sites, taps = S.oracle("full_block")
    assert c.D % 2 == 1 and S.out_dims(c.D, c.H, c.W)[0] == 3
    assert int(taps.max()) == 27 and int((taps == 27).sum()) >= c.B
    assert len(sites) == taps.size                  # every output site is active
    assert len(c.coord) == c.B * c.D * c.H * c.W


def test_corners_faces_reaches_every_side_of_the_grid():
    c = S.case("corners_faces")
    sites, taps = S.oracle("corners_faces")
    Do, Ho, Wo = S.out_dims(c.D, c.H, c.W)
    assert c.D % 2 == 0 and Do == 2
    have = {tuple(r) for r in c.coord.tolist()}
    for b in range(c.B):
        for z in (0, c.D - 1):
            for y in (0, c.H - 1):
                for x in (0, c.W - 1):
                    assert (b, z, y, x) in have
        dims = {1: c.D, 2: c.H, 3: c.W}
        for axis, n in dims.items():                    # a cell on each face that is on no other face
            for side in (0, n - 1):
                sel = c.coord[(c.coord[:, 0] == b) & (c.coord[:, axis] == side)].tolist()
                assert any(all(0 < r[a] < m - 1 for a, m in dims.items() if a != axis) for r in sel), (b, axis, side)
        for d, lim in ((1, Do), (2, Ho), (3, Wo)):      # active sites on both faces of every output axis
            on = sites[sites[:, 0] == b][:, d]
            assert on.min() == 0 and on.max() == lim - 1
    assert int((c.coord[:, 1] == c.D - 1).sum()) >= 2 * 5       # the last depth plane (odd z: two output depths asked, one exists)


def test_batch_seam_is_the_two_cells_either_side_of_the_item_boundary():
    c = S.case("batch_seam")
    sites, taps = S.oracle("batch_seam")
    Do, Ho, Wo = S.out_dims(c.D, c.H, c.W)
    assert sorted(c.coord.tolist()) == [[0, c.D - 1, c.H - 1, c.W - 1], [1, 0, 0, 0]]
    # z = 3 of D = 4: output depths (3 + 1 - kd) / 2 in {2 (out of range), 1}: 1 x 2 x 2 sites; z = 0: depth 0, 2 x 2 sites
    assert len(sites) == 8 and int(taps.max()) == 1
    assert {tuple(s) for s in sites[sites[:, 0] == 0].tolist()} == {(0, Do - 1, h, w) for h in (Ho - 2, Ho - 1) for w in (Wo - 2, Wo - 1)}
    assert {tuple(s) for s in sites[sites[:, 0] == 1].tolist()} == {(1, 0, h, w) for h in (0, 1) for w in (0, 1)}


def test_one_item_empty_and_the_two_smallest():
    c = S.case("one_item_empty")
    sites, _ = S.oracle("one_item_empty")
    assert (c.coord[:, 0] == 1).all() and len(sites) > 0 and (sites[:, 0] == 1).all()
    c = S.case("single")
    sites, taps = S.oracle("single")
    assert len(c.coord) == 1 and c.coord[0, 1] % 2 == 1 and len(sites) == S.PER_VOXEL and int(taps.max()) == 1
    assert S.list_cap(c) == S.PER_VOXEL
    c = S.case("empty")
    sites, taps = S.oracle("empty")
    assert len(c.coord) == 0 and len(sites) == 0 and int(taps.max()) == 0 and S.list_cap(c) == 1


def test_depth_parity_has_one_isolated_voxel_at_every_depth():
    c = S.case("depth_parity")
    sites, taps = S.oracle("depth_parity")
    Do = S.out_dims(c.D, c.H, c.W)[0]
    assert sorted(c.coord[:, 1].tolist()) == list(range(10)) and Do == 5
    assert int(taps.max()) == 1                      # no output site sees two voxels
    vox, tap = S.single_tap("depth_parity")
    for v, (b, z, y, x) in enumerate(c.coord.tolist()):
        mine = sites[vox == v]
        depths = sorted(set(mine[:, 1].tolist()))
        want = [z // 2] if z % 2 == 0 else [d for d in ((z - 1) // 2, (z + 1) // 2) if d < Do]
        assert depths == want, (z, depths)
        assert len(mine) == 9 * len(want) or y in (0, c.H - 1) or x in (0, c.W - 1), (z, len(mine))
    assert sorted(set(sites[vox == int(np.flatnonzero(c.coord[:, 1] == 9)[0])][:, 1].tolist())) == [4]   # z = 9: upper tap outside


@pytest.mark.parametrize("n", S.COUNT_TARGETS)
def test_count_cases_have_exactly_that_many_active_sites(n):
    c = S.case(f"count_{n}")
    sites, taps = S.oracle(f"count_{n}")
    assert len(sites) == n and int(taps.max()) == 1
    assert S.list_cap(c) > n                         # the list is not cut
    tile = S.LIST_TILE if n > 128 else S.RB_ROWS
    assert n % tile in (tile - 1, 0, 1)


@pytest.mark.parametrize("k", S.K_TARGETS)
def test_k_cases_have_exactly_that_many_voxels_in_both_items(k):
    c = S.case(f"k_{k}")
    assert len(c.coord) == k and set(c.coord[:, 0].tolist()) == {0, 1}
    assert set(c.coord[:, 1].tolist()) == set(range(10))      # every depth, so every residue class at every depth
    sites, taps = S.oracle(f"k_{k}")
    assert int(taps.max()) >= 2                      # some sites sum more than one voxel


def test_lattice_fills_the_list_to_its_capacity_past_one_persistent_trip():
    c = S.case("lattice")
    sites, taps = S.oracle("lattice")
    K = len(c.coord)
    Do, Ho, Wo = S.out_dims(c.D, c.H, c.W)
    M = c.B * Do * Ho * Wo
    assert K == 8448
    assert len(sites) == S.PER_VOXEL * K == min(M, S.PER_VOXEL * K) == S.list_cap(c) == 152064
    assert len(sites) > S.RB_MAX_BLOCKS * S.RB_ROWS == 131072
    assert int(taps.max()) == 1
    vox, tap = S.single_tap("lattice")
    assert vox.min() == 0 and vox.max() == K - 1 and (np.bincount(vox) == S.PER_VOXEL).all()
    assert tap.min() >= 0 and tap.max() <= 26 and len(np.unique(tap)) == 18      # kd = 1 never lands on a site for odd z


def test_scan_carry_needs_a_second_trip_of_the_tile_sum_scan():
    c = S.case("scan_carry")
    sites, taps = S.oracle("scan_carry")
    Do, Ho, Wo = S.out_dims(c.D, c.H, c.W)
    M = c.B * Do * Ho * Wo
    assert len(c.coord) == 4000 and M == 563200
    assert -(-M // S.SCAN_TILE) == 275 > S.SCAN_WIDTH
    assert (sites[:, 0] * Do * Ho * Wo + sites[:, 1] * Ho * Wo + sites[:, 2] * Wo + sites[:, 3]).max() >= S.SCAN_WIDTH * S.SCAN_TILE
    assert len(sites) < S.list_cap(c)
