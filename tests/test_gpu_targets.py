"""Device RPN target generation (csrc/targets.hip through vn_rpn_targets / voxelnet_amd.targets) against the oracle
(oracle/targets.py, itself pinned to the reference by tests/golden/targets_car.npz) and against that fixture directly.
Bar: which anchors are positive / negative — bit-exact; regression targets — the float64 oracle values rounded to
float32, within 1 float32 ulp (the device's float64 log may differ from glibc's in the last float64 bit).

Off the Car grid (tests/label_cases.py; what each case contains is asserted on the oracle alone by
tests/test_label_cases_host.py): the Pedestrian and Cyclist constants, anchor grids of 2 to 810 anchors that leave partial
waves and workgroups, a grid tiled three times so that every arg-max is tied across workgroups.  The oracle for those
classes is the Car-pinned code with the other classes' constants; there is no golden of their own.  Same bars."""
import os

import numpy as np
import pytest
import torch

import label_cases as L
from oracle import targets as ot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "targets_car.npz")


def _check(pos, neg, tgt, ref_pos, ref_neg, ref_tgt):
    assert pos.dtype == torch.float32 and tgt.dtype == torch.float32
    assert np.array_equal(pos.cpu().numpy(), ref_pos.astype(np.float32))
    assert np.array_equal(neg.cpu().numpy(), ref_neg.astype(np.float32))
    t, r = tgt.cpu().numpy(), ref_tgt.astype(np.float32)
    assert np.array_equal(t != 0, r != 0)
    np.testing.assert_allclose(t, r, rtol=1.2e-7, atol=0)


def test_targets_match_reference_fixture():
    from voxelnet_amd import targets as T
    g = np.load(GOLD, allow_pickle=False)
    n = int(g["n_samples"])
    labels = [[str(s) for s in g[f"labels{b}"]] for b in range(n)]
    shape = tuple(int(v) for v in g["shape"])
    gen = T.TargetGenerator("Car", DEV)
    assert np.array_equal(gen.anchors, ot.generate_anchors("Car"))           # bit-identical anchors
    pos, neg, tgt = gen(labels, shape)
    assert pos.shape == (n, *shape, 2) and neg.shape == (n, *shape, 2) and tgt.shape == (n, *shape, 14)
    for b in range(n):
        assert np.array_equal(np.flatnonzero(pos[b].cpu().numpy()).astype(np.int32), g[f"pos_idx{b}"]), b
        assert np.array_equal(np.packbits(neg[b].cpu().numpy().reshape(-1).astype(np.uint8)), g[f"neg_bits{b}"]), b
        t = tgt[b].cpu().numpy().reshape(-1)
        nz = np.flatnonzero(t)
        assert np.array_equal(nz.astype(np.int32), g[f"tgt_idx{b}"]), b
        np.testing.assert_allclose(t[nz], g[f"tgt_val{b}"].astype(np.float32), rtol=1.2e-7, atol=0)
    # module-level function with the reference's signature
    p2, n2, t2 = T.generate_targets(labels, shape, gen.anchors, "Car", "lidar", DEV)
    assert torch.equal(p2, pos) and torch.equal(n2, neg) and torch.equal(t2, tgt)


@pytest.mark.parametrize("seed,counts", [(1, [3, 0, 40]), (2, [1]), (3, [128, 7])])
def test_targets_match_oracle_on_random_boxes(seed, counts):
    """boxes straight in lidar coordinates: dense scenes, duplicates (ties between boxes), boxes outside the range"""
    from voxelnet_amd import targets as T
    rng = np.random.default_rng(seed)
    boxes = []
    for c in counts:
        b = np.stack([rng.uniform(-5, 75, c), rng.uniform(-45, 45, c), rng.uniform(-2, -1, c), rng.uniform(1.3, 1.8, c),
                      rng.uniform(1.4, 1.9, c), rng.uniform(3.2, 4.6, c), rng.uniform(-1.57, 1.57, c)], axis=1)
        if c >= 3:
            b[1] = b[0]                      # identical boxes: the first one must win every tie
        boxes.append(b)
    anchors = ot.generate_anchors("Car")
    ref = ot.generate_targets_from_boxes(boxes, (200, 176), anchors, "Car")
    gen = T.TargetGenerator("Car", DEV)
    _check(*gen.from_boxes(boxes), *ref)
    with pytest.raises(T._lib.VoxelnetHipError):
        gen.from_boxes([np.zeros((129, 7))])


def test_host_helpers_match_oracle():
    from voxelnet_amd import targets as T
    g = np.load(GOLD, allow_pickle=False)
    labels = [[str(s) for s in g[f"labels{b}"]] for b in range(int(g["n_samples"]))]
    for a, b in zip(T.label_to_gt_box_3d(labels, "Car"), ot.label_to_gt_box_3d(labels, "Car")):
        assert np.array_equal(a, b)
        assert np.array_equal(T.gt_standup_boxes(a), ot.gt_standup_2d(b))
    for cls in ("Car", "Pedestrian", "Cyclist"):
        assert np.array_equal(T.generate_anchors(cls), ot.generate_anchors(cls))


def test_rpn3d_forward_generates_targets_from_labels():
    """RPN3D.forward(batch, device) with label lines in x[1] == the same call with the oracle's targets passed in"""
    from voxelnet_amd import model as M
    from voxelnet_amd import synth
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.voxelize import voxelize_device
    g = np.load(GOLD, allow_pickle=False)
    labels = [[str(s) for s in g["labels0"]]]
    M.set_precision("bf16")
    torch.manual_seed(3)
    model = M.RPN3D("Car").to(DEV).train(True)
    grid = grid_config("Car")
    f, c, _ = voxelize_device(torch.from_numpy(synth.workload_frames(1, batch=1)[0]).to(DEV), grid, 0, coord_cols=4)
    batch = (None, labels, [f], None, [c], None, None)
    out = model(batch, DEV)
    ref_t = ot.generate_targets(labels, (200, 176), ot.generate_anchors("Car"))
    # (train-mode BatchNorm updates running stats only: the two forwards see the same weights)
    out2 = model(batch, DEV, targets=tuple(torch.from_numpy(a.astype(np.float32)).to(DEV) for a in ref_t))
    for a, b in zip(out[2:], out2[2:]):
        assert abs(a.item() - b.item()) <= 1e-6 * max(1.0, abs(b.item()))
    assert model.anchors.shape == (200, 176, 2, 7)


# ------------------------------------------------------------------------------------- off the Car anchor grid
_CASES = L.all_target_cases()


@pytest.mark.parametrize("case", _CASES, ids=[c.id for c in _CASES])
def test_targets_match_oracle_off_the_car_grid(case):
    """every element of the three maps is compared (from_boxes returns exactly (B,h,w,.) tensors): a tail thread that
    skipped the last anchors, or a class constant wired to the wrong field, shows"""
    from voxelnet_amd import targets as T
    gen = T.TargetGenerator(case.cls_name, DEV, anchors=None if case.grid == "full" else case.anchors)
    assert np.array_equal(gen.anchors, case.anchors) and gen.n_anchors == case.n_anchors
    pos, neg, tgt = gen.from_boxes(case.boxes)
    B = len(case.counts)
    assert pos.shape == (B, *case.shape, 2) and neg.shape == (B, *case.shape, 2) and tgt.shape == (B, *case.shape, 14)
    _check(pos, neg, tgt, *case.ref)
    if case.grid == "tiled":
        # each box's best IoU is reached in all three copies: its arg-max positive sits in the FIRST one
        n1 = case.n_anchors // L.TILES
        c = ot.CLASSES[case.cls_name]
        ph, found = pos.cpu().numpy().reshape(B, -1), 0
        for b, iou in enumerate(case.iou):
            if iou.shape[1] == 0:
                assert not ph[b].any()
                continue
            only = np.flatnonzero((ph[b] == 1) & ~(iou > c["pos"]).any(axis=1))
            assert (only < n1).all(), (b, only)
            found += len(only)
        assert found >= 1


@pytest.mark.parametrize("cls", ["Pedestrian", "Cyclist"])
def test_label_route_for_the_other_classes(cls):
    """label lines of the class with lines of five other classes mixed in; the second call comes out of the label cache"""
    from voxelnet_amd import targets as T
    case = L.target_case(cls, "full", *L.FULL_SEEDS[0])
    labels = [L.label_lines(cls, b, 10 + i) for i, b in enumerate(case.boxes)]
    ref = ot.generate_targets(labels, case.shape, ot.generate_anchors(cls), cls)
    assert ref[0].sum() >= 1
    gen = T.TargetGenerator(cls, DEV)
    first = gen(labels, case.shape)
    _check(*first, *ref)
    assert not T._LABEL_CACHE or len(gen._parsed) == len(labels)
    second = gen(labels)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    third = T.generate_targets(labels, case.shape, case.anchors, cls, "lidar", DEV)
    for a, b in zip(first, third):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(T._lib.VoxelnetHipError):
        gen.from_boxes([np.zeros((129, 7))])          # more than VN_TARGETS_MAX_GT boxes


def test_targets_leave_what_follows_their_maps_untouched():
    """vn_rpn_targets called directly on the N = 270 grid (one workgroup plus 14 anchors) with pos / neg / targets as views
    into LARGER buffers pre-filled with a sentinel: what follows the B*N (B*N*7) elements the call owns stays as it was"""
    from voxelnet_amd import _lib
    from voxelnet_amd import targets as T
    case = L.target_case("Pedestrian", L.SLICE_SHAPES[-1], *L.SLICE_SEEDS[0])
    gen = T.TargetGenerator("Pedestrian", DEV, anchors=case.anchors)
    B, N, G = len(case.counts), case.n_anchors, max(case.counts)
    assert N == 270
    gt = np.zeros((B, G, 7), dtype=np.float64)
    g2 = np.zeros((B, G, 4), dtype=np.float32)
    for b, boxes in enumerate(case.boxes):
        gt[b, :len(boxes)] = boxes
        g2[b, :len(boxes)] = ot.gt_standup_2d(boxes).reshape(-1, 4)
    gt_d, g2_d = torch.from_numpy(gt).to(DEV), torch.from_numpy(g2).to(DEV)
    cnt_d = torch.tensor(case.counts, dtype=torch.int32, device=DEV)
    SENTINEL, EXTRA = -7.0, 4096
    bufs = [torch.full((B * N * k + EXTRA,), SENTINEL, dtype=torch.float32, device=DEV) for k in (1, 1, 7)]
    pos, neg, tgt = (buf[:B * N * k] for buf, k in zip(bufs, (1, 1, 7)))
    nbytes = _lib.load().vn_rpn_targets_workspace_bytes(B, N, G)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    cfg = T.CLASS_CFG["Pedestrian"]
    with _lib.on_device(torch.device(DEV)):
        _lib.call("vn_rpn_targets", gen._anchors_dev.data_ptr(), N, gt_d.data_ptr(), g2_d.data_ptr(), cnt_d.data_ptr(), B, G,
                  float(cfg["pos_iou"]), float(cfg["neg_iou"]), float(cfg["h"]), pos.data_ptr(), neg.data_ptr(), tgt.data_ptr(),
                  ws.data_ptr(), nbytes, _lib.raw_stream())
    torch.cuda.synchronize()
    for buf, k in zip(bufs, (1, 1, 7)):
        assert (buf[B * N * k:] == SENTINEL).all()
        assert (buf[:B * N * k] != SENTINEL).all()          # and every element it owns was written
    _check(pos.view(B, *case.shape, 2), neg.view(B, *case.shape, 2), tgt.view(B, *case.shape, 14), *case.ref)


def test_rpn3d_pedestrian_targets_raise_about_the_anchor_grid():
    """the reference's own mismatch (model.py: the network emits 200 x 240 maps, the anchor grid and rpn_output_shape say
    100 x 120): an error, not targets that fit no map"""
    from voxelnet_amd import model as M
    model = M.RPN3D("Pedestrian")
    assert tuple(model.rpn_output_shape) == (100, 120)
    case = L.target_case("Pedestrian", "full", *L.FULL_SEEDS[0])
    labels = [L.label_lines("Pedestrian", b, 10 + i) for i, b in enumerate(case.boxes)]
    with pytest.raises(M._lib.VoxelnetHipError, match="anchor grid"):
        model._target_generator(DEV)(labels)
