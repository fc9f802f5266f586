"""CPU: the anchor mask's host side — the guards of tests/anchor_mask_cases.py on the reference
alone, voxelnet_amd.anchor_mask.anchor_cell_rects against the restatement with the other operation order, the two
reference counts against each other, the status codes of the entry points without a GPU, the Python argument errors,
and that the option leaves a default model as it is."""
import ctypes

import numpy as np
import pytest
import torch

import anchor_mask_cases as C
import anchor_mask_ref as R
from oracle import targets as ot

CLASSES = ("Car", "Pedestrian", "Cyclist")
ON_BOUNDARY = {"Car": 1504, "Pedestrian": 880, "Cyclist": 0}          # rectangle edges exactly on a cell boundary


def _stock(cls_name):
    from voxelnet_amd.config import grid_config
    return ot.generate_anchors(cls_name), grid_config(cls_name)


@pytest.fixture(scope="module")
def stock_tables():
    return {c: R.rects(*_stock(c)) for c in CLASSES}


def test_guard_no_edge_between_the_snap_and_ordinary_values():
    """on the reference alone: for the stock anchors of the three classes and every hand-made set, no rectangle edge lies
    in (1e-9, 1e-6) cells of a cell boundary — the snap decides nothing that float64 noise could decide otherwise"""
    sets = {c: _stock(c) for c in CLASSES}
    sets.update(C.hand_anchors())
    for name, (anchors, grid) in sets.items():
        gap, on = C.min_unsnapped_gap(anchors, grid)
        print(f"{name}: {on} edges on a boundary, nearest other edge {gap:.3e} cells")
        assert gap >= 1e-6, (name, gap)
        if name in ON_BOUNDARY:
            assert on == ON_BOUNDARY[name], (name, on)
    assert C.min_unsnapped_gap(*C.hand_anchors()["on_boundaries"])[1] == 16


def test_cell_rects_equal_the_restatement(stock_tables):
    from voxelnet_amd.anchor_mask import anchor_cell_rects
    for c in CLASSES:
        anchors, grid = _stock(c)
        got, ref = anchor_cell_rects(anchors, grid), stock_tables[c]
        assert got.dtype == np.int32 and got.shape == (anchors.size // 7, 4) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, ref), c
        assert (ref[:, 2] >= ref[:, 0]).all() and (ref[:, 3] >= ref[:, 1]).all(), c          # no stock anchor is empty
        assert ref.min() >= 0 and ref[:, 2].max() <= grid.W - 1 and ref[:, 3].max() <= grid.H - 1
    for name, (anchors, grid) in C.hand_anchors().items():
        got, ref = anchor_cell_rects(anchors, grid), R.rects(anchors, grid)
        assert np.array_equal(got, ref), (name, got, ref)
    # by hand: l = 0.8, w = 0.4 centred on (1.0, 1.0) m of the grid covers cells w 3..6, h 4..5; quarter-turned w 4..5, h 3..6
    a, g = C.hand_anchors()["on_boundaries"]
    assert anchor_cell_rects(a, g)[:2].tolist() == [[3, 4, 6, 5], [4, 3, 5, 6]]
    a, g = C.hand_anchors()["outside_or_empty"]
    assert anchor_cell_rects(a, g)[:5].tolist() == [[0, 0, -1, -1]] * 5
    bad = np.array(a, copy=True)
    bad[0, 0, 0, 0] = np.nan
    bad[0, 0, 1, 5] = np.inf
    assert anchor_cell_rects(bad, g)[:2].tolist() == [[0, 0, -1, -1]] * 2


@pytest.mark.parametrize("hw", list(C.GRIDS), ids=lambda s: "x".join(str(v) for v in s))
def test_brute_force_and_cumsum_references_agree(hw):
    H, W = hw
    coord, rect = C.voxels(H, W), C.rect_table(H, W)
    brute, cs = R.count_brute(coord, C.B, H, W, rect), R.count_cumsum(coord, C.B, H, W, rect)
    assert np.array_equal(brute, cs)
    assert brute[0, 3] == R.valid_rows(coord, C.B, H, W)[:, 0].tolist().count(0) and brute[1].max() == 0 and brute[2, 3] == 1
    assert brute[0, 9] == 0 and brute[0].max() >= min(C.D, 6) and len(R.valid_rows(coord, C.B, H, W)) == len(coord) - 4
    empty = np.zeros((0, 4), dtype=np.int64)
    assert not R.count_brute(empty, C.B, H, W, rect).any() and not R.count_cumsum(empty, C.B, H, W, rect).any()


def test_status_codes_without_a_gpu():
    from voxelnet_amd import _lib
    lib = _lib.load()
    assert lib.vn_anchor_mask_workspace_bytes(2, 400, 352, 70400) > 0
    for bad in ((0, 400, 352, 70400), (2, 0, 352, 70400), (2, 400, -1, 70400), (2, 400, 352, 0), (-2, 400, 352, 70400)):
        assert lib.vn_anchor_mask_workspace_bytes(*bad) == 0, bad
    assert lib.vn_anchor_mask_workspace_bytes(2, 1 << 14, 1 << 14, 70400) == 0
    assert lib.vn_anchor_mask(None, 10, 2, 16, 24, None, 192, 1, None, None, None, None, None, 0, None) == -1      # VN_EINVAL
    assert lib.vn_anchor_mask_probs(None, None, 2, 192, _lib.VN_DETECT_FLAT, None, None) == -1
    # pointers that pass the checks (host memory: nothing is launched before the workspace size is compared)
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) // 256 * 256
    need = lib.vn_anchor_mask_workspace_bytes(2, 16, 24, 192)
    assert need > 0
    args = lambda K, thr, pos, neg, nbytes: lib.vn_anchor_mask(p, K, 2, 16, 24, p, 192, thr, p, None, pos, neg, p, nbytes, None)  # noqa: E731
    assert args(10, 1, None, None, need - 1) == -3                                                                  # VN_EWORKSPACE
    assert args(10, 1, None, None, 0) == -3
    assert args(10, -1, None, None, need) == -1 and args(-1, 1, None, None, need) == -1 and args(1 << 31, 1, None, None, need) == -1
    assert args(10, 1, p, None, need) == -1 and args(10, 1, None, p, need) == -1                                    # pos and neg are a pair
    assert lib.vn_anchor_mask(None, 10, 2, 16, 24, p, 192, 1, p, None, None, None, p, need, None) == -1            # K > 0 needs coord
    assert lib.vn_anchor_mask(p, 10, 2, 16, 24, p + 4, 192, 1, p, None, None, None, p, need, None) == -2           # misaligned table
    assert lib.vn_anchor_mask_probs(p, p, 2, 192, 7, p + 4096, None) == -1                                           # unknown layout
    assert lib.vn_anchor_mask_probs(p, p, 2, 191, _lib.VN_DETECT_SITE, p + 4096, None) == -1                         # odd N by site
    assert lib.vn_anchor_mask_probs(p, p, 2, 192, _lib.VN_DETECT_FLAT, p, None) == -1                                # out aliases probs
    assert lib.vn_anchor_mask_probs(p, p, 2, 192, _lib.VN_DETECT_FLAT, p + 4, None) == -1


def test_python_argument_errors():
    from voxelnet_amd import _lib
    from voxelnet_amd import model as M
    from voxelnet_amd.anchor_mask import AnchorMasker, check_threshold, mask_probs
    from voxelnet_amd.predict import BoxDecoder
    from voxelnet_amd.targets import TargetGenerator
    for bad in (-1, 1.5, "1", True, None):
        with pytest.raises(ValueError):
            check_threshold(bad)
    assert check_threshold(0) == 0 and check_threshold(np.int64(5)) == 5
    with pytest.raises(ValueError):
        AnchorMasker("Car", "cuda:0", threshold=-1)
    with pytest.raises(ValueError):
        M.RPN3D("Car", anchor_area_threshold=-1)
    with pytest.raises(ValueError):
        M.RPN3D("Car", anchor_area_threshold=0.5)
    with pytest.raises(_lib.VoxelnetHipError):
        AnchorMasker("Car", "cpu")
    with pytest.raises(_lib.VoxelnetHipError):
        mask_probs(torch.zeros(2, 2, 8, 12), torch.ones(2, 8, 12, 2, dtype=torch.uint8), 192, _lib.VN_DETECT_FLAT)
    # the methods check their arguments before anything touches a device: objects made without their device state
    mk = AnchorMasker.__new__(AnchorMasker)
    mk.shape, mk.n_anchors, mk.threshold, mk.grid = (8, 12), 192, 1, C.tiny_grid()
    with pytest.raises(_lib.VoxelnetHipError):
        mk.mask(torch.zeros(5, 4, dtype=torch.int64), 2)
    with pytest.raises(ValueError):
        mk.mask_probs(torch.zeros(2, 2, 8, 12), torch.ones(2, 8, 12, 2, dtype=torch.uint8), layout="rows")
    dec = BoxDecoder.__new__(BoxDecoder)
    dec.layout, dec.n_anchors = "flat", 192
    probs, deltas, m = torch.zeros(2, 2, 8, 12), torch.zeros(2, 14, 8, 12), torch.ones(2, 8, 12, 2, dtype=torch.uint8)
    for thr in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="score_thres"):
            dec.decode_device(probs, deltas, score_thres=thr, anchor_mask=m)
        with pytest.raises(ValueError, match="score_thres"):
            dec.candidates_device(probs, deltas, thr, 64, anchor_mask=m)
    with pytest.raises(_lib.VoxelnetHipError):
        dec.decode_device(probs, deltas, score_thres=0.5, anchor_mask=m)
    gen = TargetGenerator.__new__(TargetGenerator)
    gen.n_anchors = 192
    with pytest.raises(_lib.VoxelnetHipError):
        gen._apply_mask((torch.zeros(2, 8, 12, 2), torch.zeros(2, 8, 12, 2), torch.zeros(2, 8, 12, 14)), m)


def test_default_model_is_untouched():
    """RPN3D() and RPN3D(anchor_area_threshold=None) have the 104 parameters and the reference's keys; the option adds no
    parameter or state_dict key, is a class-level default (old pickles load) and its caches do not travel"""
    from oracle import torch_ref as tr
    from voxelnet_amd import model as M
    ref = tr.make_state_dict("Car")
    for m in (M.RPN3D(), M.RPN3D(anchor_area_threshold=None), M.RPN3D(anchor_area_threshold=1)):
        sd = m.state_dict()
        assert set(sd) == set(ref) and len(list(m.parameters())) == 104
        assert sum(p.numel() for p in m.parameters()) == 6809392
    m = M.RPN3D()
    assert m.anchor_area_threshold is None and "anchor_area_threshold" not in m.__dict__ and m.last_anchor_mask is None
    on = M.RPN3D(anchor_area_threshold=1)
    assert on.anchor_area_threshold == 1
    on.__dict__["_maskers"], on.last_anchor_mask = {1: object()}, torch.zeros(1)
    st = on.__getstate__()
    assert "_maskers" not in st and "last_anchor_mask" not in st and st["anchor_area_threshold"] == 1
    assert M.RPN3D.anchor_area_threshold is None and {"_maskers", "last_anchor_mask"} <= set(M.RPN3D._RUNTIME_KEYS)
