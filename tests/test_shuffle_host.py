"""CPU: the host half of the device point shuffle (voxelnet_amd/shuffle.py, csrc/shuffle.hip) — the restatement
tests/shuffle_ref.py against the specification's test vectors and against what a shuffle has to be (a permutation that
spreads), the index draw against np.random.shuffle of the cloud itself (same rows, same Mersenne-Twister state), the key
draw, the status codes of the two entry points that need no launch to decide, and the pipeline's switch."""
import ctypes

import numpy as np
import pytest

import shuffle_ref as R

KEYS = [1, 2, 3, 4, 5, 6]


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_restatement_gives_the_specified_vectors():
    assert R.permutation(5, KEYS).tolist() == [4, 2, 0, 3, 1]
    assert R.permutation(257, KEYS)[:8].tolist() == [231, 24, 86, 110, 182, 104, 64, 95]
    assert [R.half_bits(n) for n in (1, 2, 4, 5, 16, 17, 257, 65536, 65537, 2 ** 31 - 1)] == [1, 1, 1, 2, 2, 3, 5, 8, 9, 16]
    assert int(R.fmix32(1)) == 0x514E28B7 and int(R.fmix32(0)) == 0          # MurmurHash3's finalizer


@pytest.mark.parametrize("n", [1, 2, 3, 5, 255, 256, 257, 1023, 1025, 4097, 65536, 65537, 20000])
def test_restatement_is_a_permutation(n):
    for keys in (KEYS, [0] * 6, [0xFFFFFFFF] * 6, np.random.RandomState(n).randint(0, 2 ** 32, 6, dtype=np.uint64)):
        steps = []
        p = R.permutation(n, keys, steps)
        assert p.shape == (n,) and np.array_equal(np.sort(p), np.arange(n)), (n, keys)
        assert steps[0] <= 64                                # the domain is below 4n: walks stay short


def _spread(perm_of):
    """chi-square (10 equal bins, 9 degrees of freedom) of the source row of output rows 0, 1, 500, 999, and the mean
    number of i with p(i+1) == p(i) + 1, over 4,000 key sets at n = 1000"""
    rs = np.random.RandomState(0)
    n, sets = 1000, 4000
    rows = (0, 1, 500, 999)
    hist = np.zeros((len(rows), 10))
    adjacent = 0
    for _ in range(sets):
        p = perm_of(n, rs.randint(0, 2 ** 32, 6, dtype=np.uint64))
        for j, r in enumerate(rows):
            hist[j, p[r] * 10 // n] += 1
        adjacent += int((p[1:] == p[:-1] + 1).sum())
    expect = sets / 10
    return ((hist - expect) ** 2 / expect).sum(1), adjacent / sets


def test_the_bijection_spreads_and_the_conditions_reject_what_does_not():
    chi2, adjacent = _spread(R.permutation)
    print("chi2 of rows 0, 1, 500, 999:", np.round(chi2, 1), " mean adjacent pairs:", round(adjacent, 3))
    assert (chi2 < 27.88).all(), chi2                        # the 0.1 % point at 9 degrees of freedom
    assert 0.9 <= adjacent <= 1.1, adjacent                  # expected (n - 1) / n = 0.999
    # a permutation that does not shuffle fails both conditions: the identity, and a rotation
    for bad in (lambda n, keys: np.arange(n), lambda n, keys: (np.arange(n) + 337) % n):
        chi2, adjacent = _spread(bad)
        assert (chi2 >= 27.88).any() and not 0.9 <= adjacent <= 1.1, (chi2, adjacent)


@pytest.mark.parametrize("n", [1, 2, 257, 20000])
def test_draw_index_is_the_shuffle_of_the_cloud(n):
    from voxelnet_amd import shuffle as S
    cloud = np.random.default_rng(n).standard_normal((n, 7)).astype(np.float32)
    want = cloud.copy()
    np.random.seed(1000 + n)
    np.random.shuffle(want)
    after = np.random.get_state()
    np.random.seed(1000 + n)
    index = S.draw_index(n)
    assert index.dtype == np.int32 and index.shape == (n,) and np.array_equal(np.sort(index), np.arange(n))
    assert np.array_equal(cloud[index], want)
    assert _same_state(np.random.get_state(), after)
    assert np.array_equal(R.permute_points(cloud[:, :4], index), want[:, :4])
    assert S.draw_index(0).shape == (0,) and S.draw_index(0).dtype == np.int32


def test_draw_keys_is_one_randint_of_six_uint32(monkeypatch):
    from voxelnet_amd import shuffle as S
    np.random.seed(5)
    want = np.random.randint(0, 2 ** 32, 6, dtype=np.uint32)
    after = np.random.get_state()
    calls = []
    real = np.random.randint
    monkeypatch.setattr(np.random, "randint", lambda *a, **k: (calls.append((a, k)), real(*a, **k))[1])
    np.random.seed(5)
    keys = S.draw_keys()
    assert calls == [((0, 2 ** 32, 6), {"dtype": np.uint32})]
    assert keys.dtype == np.uint32 and keys.shape == (6,) and np.array_equal(keys, want)
    assert _same_state(np.random.get_state(), after)


def test_entry_points_check_their_arguments_on_the_host():
    """status codes that need no device work to decide (the conventions of vn_gt_paste); none of these launches"""
    from voxelnet_amd import _lib
    lib = _lib.load()
    keys = (ctypes.c_uint32 * 6)(*KEYS)
    k = ctypes.addressof(keys)
    E, U = -1, -2
    perm, shuf = lib.vn_permute_points, lib.vn_shuffle_points
    for call, third in ((perm, 0x40000), (shuf, k)):
        assert call(None, 10, third, 0x2000, None) == E                       # null pointers with n > 0
        assert call(0x1000, 10, None, 0x2000, None) == E
        assert call(0x1000, 10, third, None, None) == E
        assert call(0x1000, -1, third, 0x2000, None) == E
        assert call(0x1000, 1 << 31, third, 0x100000000000, None) == E        # n > 2^31 - 1
        assert call(0x1004, 10, third, 0x2000, None) == U                     # 4-byte-offset pointers
        assert call(0x1000, 10, third, 0x2008, None) == U
        assert call(0x1000, 10, third, 0x1000, None) == E                     # a gather cannot run in place
        assert call(0x1000, 10, third, 0x1000 + 9 * 16, None) == E            # the last input row is the first output row
        assert call(0x1000 + 9 * 16, 10, third, 0x1000, None) == E
        assert call(None, 0, None, None, None) == 0                           # n == 0: a no-op
        assert call(0x1004, 0, None, 0x1004, None) == 0
    assert perm(0x1000, 10, 0x40002, 0x2000, None) == U                       # a table off its 4-byte alignment
    assert perm(0x1000, 10, 0x2000 + 9 * 16 + 12, 0x2000, None) == E          # the table inside out
    assert sorted(n for n in _lib.SIGNATURES if "e_points" in n) == ["vn_permute_points", "vn_shuffle_points"]
    assert lib.vn_abi_version() == 4


def test_no_cpu_path_for_the_points():
    import torch
    from voxelnet_amd import _lib
    from voxelnet_amd import shuffle as S
    cloud = torch.zeros((8, 4))
    for fn in (S.enqueue_permute_points, S.permute_points_device):
        with pytest.raises(_lib.VoxelnetHipError):
            fn(cloud, np.arange(8, dtype=np.int32))
    for fn in (S.enqueue_shuffle_points, S.shuffle_points_device):
        with pytest.raises(_lib.VoxelnetHipError):
            fn(cloud, np.array(KEYS, dtype=np.uint32))


def test_an_unknown_shuffle_mode_is_refused_at_construction():
    """strings are truthy: before the switch existed, any string meant the host shuffle"""
    from voxelnet_amd import _lib
    from voxelnet_amd import dataset as D
    for bad in ("nonsense", "Index", "", None, 2):
        with pytest.raises(ValueError):
            D.DeviceCollate("cuda:0", "Car", shuffle_points=bad)
        with pytest.raises(ValueError):
            D.DeviceBatcher([], "cuda:0", "Car", shuffle_points=bad)
    # the known values get as far as the device check (this process has no HIP device to give them)
    for ok in (True, False, "host", "index", "device"):
        with pytest.raises(_lib.VoxelnetHipError):
            D.DeviceCollate("cpu", "Car", shuffle_points=ok)
