"""GPU: target assignment by a real IoU (csrc/targets_iou.hip through vn_rpn_targets_iou / targets.TargetGenerator(assign=))
against the restatement tests/assign_ref.py.

Bars.  The guard is asserted ON THE REFERENCE ALONE first (assign_cases.MARGIN = 1e-7, tests/test_gpu_detect.py's: two orders
above the 1e-9 device / reference agreement of the pair function): no best IoU within the margin of a threshold, no two
anchors (boxes) within the margin of a box's (an anchor's) best unless they tie by construction.  Then pos, neg and matched
must be equal exactly, and the regression targets are held to tests/test_gpu_targets.py's bar: the same elements non-zero,
the float64 reference values rounded to float32 within 1 float32 ulp (rtol 1.2e-7, atol 0).

Shapes (tests/assign_cases.py): 2, 130, 256, 270 anchors (less than a wave, a partial workgroup, exactly one, one plus 14),
the 270-anchor grid tiled three times (every arg-max tied across workgroups), 128 boxes on 130 anchors, the full Car grid,
Pedestrian anchors; B = 3 with (5, 0, 12) boxes; both kinds."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import assign_cases as C
from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KIND_ID = {"standup": 1, "rotated": 2}


def _generator(case, kind, **kw):
    from voxelnet_amd import targets as T
    return T.TargetGenerator(case.cls_name, DEV, anchors=case.anchors, assign=kind, **kw)


def _check(case, kind, out):
    gap = case.guard(kind)          # on the reference alone, before the device is looked at
    print(f"{case.id} {kind}: smallest gap of the reference's decisions {gap:.3e}")
    assert gap > C.MARGIN
    pos, neg, tgt, matched = (t.cpu().numpy() for t in out)
    B, N = len(case.boxes), case.n_anchors
    assert pos.shape == (B, *case.shape, 2) and neg.shape == pos.shape and matched.shape == pos.shape
    assert tgt.shape == (B, *case.shape, 14)
    assert pos.dtype == np.float32 and neg.dtype == np.float32 and tgt.dtype == np.float32 and matched.dtype == np.int32
    for b, ref in enumerate(case.ref(kind)):
        assert np.array_equal(matched[b].reshape(N), ref["matched"]), b
        assert np.array_equal(pos[b].reshape(N), ref["pos"].astype(np.float32)), b
        assert np.array_equal(neg[b].reshape(N), ref["neg"].astype(np.float32)), b
        t, r = tgt[b].reshape(N, 7), ref["targets"]
        assert np.array_equal(t != 0, r != 0), b
        np.testing.assert_allclose(t, r, rtol=1.2e-7, atol=0)


_CASES = C.cases()


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("case", _CASES, ids=[c.id for c in _CASES])
def test_assignment_matches_reference(case, kind):
    _check(case, kind, _generator(case, kind).from_boxes(case.boxes, return_matched=True))


@pytest.mark.parametrize("kind", C.KINDS)
def test_hand_made_frames(kind):
    """competing boxes, a forced positive below pos_iou, a box outside the grid, a box with w = 0 (what each frame holds is
    asserted on the reference by tests/test_assign_host.py)"""
    h = C.hand_frames()
    out = _generator(h, kind).from_boxes(h.boxes, return_matched=True)
    _check(h, kind, out)
    pos, neg = out[0].cpu().numpy().reshape(4, -1), out[1].cpu().numpy().reshape(4, -1)
    assert pos[1].sum() == 1 and not (pos * neg).any()          # the forced positive; exclusive flags


@pytest.mark.parametrize("kind", C.KINDS)
def test_deterministic_without_matched_and_inside_its_buffers(kind):
    """two calls bit-equal; matched = NULL gives the same three maps; called directly on the 270-anchor grid with every
    output a view into a LARGER buffer pre-filled with a sentinel: what follows the elements the call owns stays as it was"""
    from voxelnet_amd import _lib
    case = _CASES[3]
    assert case.n_anchors == 270
    gen = _generator(case, kind)
    first = gen.from_boxes(case.boxes, return_matched=True)
    again = gen.from_boxes(case.boxes, return_matched=True)
    three = gen.from_boxes(case.boxes)
    assert len(three) == 3
    for x, y in zip(first, again):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for x, y in zip(first, three):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    B, N, G = len(case.boxes), case.n_anchors, max(len(b) for b in case.boxes)
    gt = np.zeros((B, G, 7))
    for b, boxes in enumerate(case.boxes):
        gt[b, :len(boxes)] = boxes
    gt_d = torch.from_numpy(gt).to(DEV)
    cnt_d = torch.tensor([len(b) for b in case.boxes], dtype=torch.int32, device=DEV)
    SENTINEL, EXTRA = -7.0, 4096
    bufs = [torch.full((B * N * k + EXTRA,), SENTINEL, dtype=torch.float32, device=DEV) for k in (1, 1, 7)]
    mbuf = torch.full((B * N + EXTRA,), -7, dtype=torch.int32, device=DEV)
    nbytes = _lib.load().vn_rpn_targets_iou_workspace_bytes(B, N, G)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    with _lib.on_device(torch.device(DEV)):
        _lib.call("vn_rpn_targets_iou", gen._anchors_dev.data_ptr(), N, gt_d.data_ptr(), cnt_d.data_ptr(), B, G, KIND_ID[kind],
                  float(case.pos_iou), float(case.neg_iou), float(case.anchor_h), bufs[0].data_ptr(), bufs[1].data_ptr(),
                  bufs[2].data_ptr(), mbuf.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
    torch.cuda.synchronize()
    for buf, k in zip(bufs, (1, 1, 7)):
        assert (buf[B * N * k:] == SENTINEL).all() and (buf[:B * N * k] != SENTINEL).all()
    assert (mbuf[B * N:] == -7).all() and (mbuf[:B * N] != -7).all()
    for buf, k, want in zip(bufs + [mbuf], (1, 1, 7, 1), first):
        assert torch.equal(buf[:B * N * k].view(torch.int32), want.reshape(-1).view(torch.int32))


def test_surface_errors_and_thresholds():
    from voxelnet_amd import _lib
    from voxelnet_amd import targets as T
    case = _CASES[1]
    with pytest.raises(ValueError):
        T.TargetGenerator("Car", DEV, assign="iou")
    with pytest.raises(ValueError):
        T.TargetGenerator("Car", DEV, assign="rotated", pos_iou=float("nan"))
    with pytest.raises(_lib.VoxelnetHipError):
        T.TargetGenerator("Car", "cpu", assign="rotated")
    with pytest.raises(ValueError):
        T.TargetGenerator("Car", DEV, anchors=case.anchors).from_boxes(case.boxes, return_matched=True)
    with pytest.raises(_lib.VoxelnetHipError):
        _generator(case, "rotated").from_boxes([np.zeros((129, 7))])
    # thresholds of the caller's: with pos_iou above every IoU only the forced positives are left, one per box with M_k > 0
    gen = _generator(case, "rotated", pos_iou=1.5, neg_iou=0.0)
    assert gen.pos_iou == 1.5 and _generator(case, "rotated").pos_iou == T.CLASS_CFG["Car"]["pos_iou"]
    pos, neg, _, matched = gen.from_boxes(case.boxes, return_matched=True)
    for b, ref in enumerate(case.ref("rotated")):
        iou = ref["iou"]
        if iou.shape[1] == 0:
            assert not pos[b].any() and neg[b].all()          # a sample without a box: every anchor negative
            continue
        assert not neg[b].any()                               # m_n < 0 never holds
        want = np.full(case.n_anchors, -1)
        M = iou.max(axis=0)
        for k in range(iou.shape[1] - 1, -1, -1):
            if M[k] > 0:
                want[int(iou[:, k].argmax())] = k
        assert np.array_equal(matched[b].cpu().numpy().reshape(-1), want), b


# ---------------------------------------------------------------------------------------------------------- the model
def _tiny(golden):
    g = golden("middle_tiny_car")
    lens = [int(x) for x in g["feat_lens"]]
    feats = [f.to(DEV) for f in torch.split(torch.from_numpy(g["features"]), lens)]
    coords = [c.to(DEV) for c in torch.split(torch.from_numpy(g["coords"]), lens)]
    return feats, coords


def _tiny_anchors():
    from voxelnet_amd.targets import generate_anchors
    return np.ascontiguousarray(generate_anchors("Car")[:8, :12])          # the 8 x 12 maps of the 10 x 16 x 24 grid


def _tiny_labels():
    import eval_ref as R
    a = _tiny_anchors().reshape(-1, 7)
    x0, x1, y0, y1 = a[:, 0].min(), a[:, 0].max(), a[:, 1].min(), a[:, 1].max()
    cars = [[(0.3, 0.35, 0.2), (0.8, 0.7, -1.3)], [(0.55, 0.45, 0.8)]]
    return [[R.label_line("Car", [x0 + fx * (x1 - x0), y0 + fy * (y1 - y0), -1.7, 1.5, 1.6, 3.9, r]) for fx, fy, r in fr]
            for fr in cars]


def _tiny_model(assign, mode="bf16"):
    from voxelnet_amd import model as M
    from voxelnet_amd.targets import TargetGenerator
    M.set_precision(mode)
    m = M.RPN3D("Car", cls_loss="focal", yaw_loss="sin", target_assign=assign)
    m.load_state_dict(tr.make_state_dict("Car"))
    m.feature_net._grid = replace(m.feature_net._grid, H=16, W=24)
    m = m.to(DEV).train()
    # the module's generator on the tiny grid's anchors (its own is the full 200 x 176 grid's)
    m.__dict__["_targets"] = TargetGenerator("Car", torch.device(DEV), anchors=_tiny_anchors(), assign=assign)
    return m


def test_rpn3d_target_assign_reaches_the_generator():
    """RPN3D(target_assign=) builds its generator with that assignment: the standalone generator's maps on the same labels,
    not the reference assignment's; an unknown string is an error at construction"""
    from voxelnet_amd import model as M
    from voxelnet_amd import targets as T
    labels = [C.round_trip_frames(T.generate_anchors("Car"))[0]]
    with pytest.raises(ValueError):
        M.RPN3D("Car", target_assign="iou")
    assert M.RPN3D("Car").target_assign == "reference"
    m = M.RPN3D("Car", target_assign="rotated")
    gen = m._target_generator(torch.device(DEV))
    assert gen.assign == "rotated" and gen is m._target_generator(torch.device(DEV)) and tuple(gen.shape) == (200, 176)
    own = gen(labels)
    alone = T.TargetGenerator("Car", DEV, assign="rotated")(labels)
    quirk = m.__class__("Car")._target_generator(torch.device(DEV))(labels)
    for x, y in zip(own, alone):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert int(own[0].sum()) >= 2 and not torch.equal(own[0], quirk[0])
    m.target_assign = "standup"          # set after construction: the next call rebuilds the generator
    assert m._target_generator(torch.device(DEV)).assign == "standup"


def test_train_step_with_rotated_assignment(golden):
    """the tiny golden batch with labels, target_assign="rotated": RPN3D.train_step as ONE call (the targets generated on the
    targets stream inside it) equals forward + backward as separate module calls bit for bit — maps, the five scalars,
    every .grad — and differs from the reference assignment's step (mirrors tests/test_gpu_focal_loss.py's check 6)"""
    from voxelnet_amd import model as M
    feats, coords = _tiny(golden)
    labels = _tiny_labels()
    batch = (None, labels, feats, None, coords, None, None)
    try:
        a = _tiny_model("rotated")
        assert a._step_fused_ok("bf16", None)
        out_a = a.train_step(batch, DEV, None)
        b = _tiny_model("rotated")
        out_b = b(batch, DEV)
        out_b[2].backward()
        c = _tiny_model("reference")
        out_c = c.train_step(batch, DEV, None)
        want = a._target_generator(torch.device(DEV))(labels)
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    assert int(want[0].sum()) >= 3 and a._target_generator(torch.device(DEV)).assign == "rotated"
    assert len(out_a) == len(out_b) == 7
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        assert torch.isfinite(x).all() and torch.equal(x, y), ("output", i)
    ga, gb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in ga:
        assert ga[k].grad is not None and torch.isfinite(ga[k].grad).all(), k
        assert torch.equal(ga[k].grad, gb[k].grad), k
    assert torch.equal(out_a[0], out_c[0]) and float(out_a[2]) != float(out_c[2])          # same maps, other targets
    # the step's loss is the loss of the standalone generator's maps
    d = _tiny_model("rotated")
    try:
        out_d = d(batch, DEV, targets=want)
    finally:
        M.set_precision("bf16")
    for x, y in zip(out_a[2:], out_d[2:]):
        assert torch.equal(x, y)
