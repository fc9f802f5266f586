"""GPU: the ATSS target assignment (csrc/targets_atss.hip through vn_rpn_targets_atss / targets.TargetGenerator(assign="atss") /
RPN3D(target_assign="atss")) against the restatement tests/atss_ref.py.

Bars.  The guard is asserted ON THE REFERENCE ALONE first (atss_cases.MARGIN = 1e-7, two orders above the 1e-9 device /
reference agreement of the pair function): no candidate cut, threshold, footprint edge or two-box tie within the margin.
Then pos, neg, matched and stats[..., 3] must be equal exactly, stats[..., :3] within 1e-9 absolute (the pair function's
agreement: mean, deviation and threshold are averages of its values), and the regression targets are held to
tests/test_gpu_assign.py's bar: the same elements non-zero, the float64 reference rounded to float32 within 1 float32 ulp.

Shapes (tests/atss_cases.py): 2, 130, 256, 270 anchors, the tiled grid (every distance tied across copies), 128 boxes on 130
anchors, the full Car grid, Pedestrian anchors, the hand-made frames, frames with copies / an invalid box / a box off the grid /
an empty sample, a 56-anchor grid with one box; top_k 1, 9, 32; both kinds.  The scan kernel cuts the sites into 1 (2 and 56
anchors), 2 (130 anchors, with 5 + 0 + 12 and with 128 boxes, and 256 anchors), 3 (270), 7 (the tiled 810: ties across chunks), 12 (the 1,536 of
the hand-made frames) and 28 (the full grid) chunks, the last one shorter wherever the sites do not divide."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import atss_cases as AC
import test_gpu_assign as GA
from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KIND_ID = {"standup": 1, "rotated": 2}
EINVAL, EWORKSPACE = -1, -3


def _generator(case, kind, top_k, **kw):
    from voxelnet_amd import targets as T
    return T.TargetGenerator(case.cls_name, DEV, anchors=case.anchors, assign="atss", atss_top_k=top_k, atss_iou=kind, **kw)


def _check(case, kind, top_k, out):
    gaps = case.guard(kind, top_k)          # on the reference alone, before the device is looked at
    print(f"{case.id} {kind} top_k {top_k}: smallest gaps of the reference's decisions {gaps}")
    assert all(g > AC.MARGIN for g in gaps.values())
    pos, neg, tgt, matched, stats = (t.cpu().numpy() for t in out)
    B, N, G = len(case.boxes), case.n_anchors, max([len(b) for b in case.boxes] + [1])
    assert pos.shape == (B, *case.shape, 2) and neg.shape == pos.shape and matched.shape == pos.shape
    assert tgt.shape == (B, *case.shape, 14) and stats.shape == (B, G, 4)
    assert pos.dtype == np.float32 and neg.dtype == np.float32 and tgt.dtype == np.float32
    assert matched.dtype == np.int32 and stats.dtype == np.float64
    for b, ref in enumerate(case.ref(kind, top_k)):
        g = ref["stats"].shape[0]
        err = float(np.abs(stats[b, :g, :3] - ref["stats"][:, :3]).max()) if g else 0.0
        print(f"  sample {b}: {int(ref['pos'].sum())} positives, stats error {err:.2e}")
        assert np.array_equal(matched[b].reshape(N), ref["matched"]), b
        assert np.array_equal(pos[b].reshape(N), ref["pos"].astype(np.float32)), b
        assert np.array_equal(neg[b].reshape(N), ref["neg"].astype(np.float32)), b
        t, r = tgt[b].reshape(N, 7), ref["targets"]
        assert np.array_equal(t != 0, r != 0), b
        np.testing.assert_allclose(t, r, rtol=1.2e-7, atol=0)
        assert err <= 1e-9, (b, err)
        assert np.array_equal(stats[b, :g, 3], ref["stats"][:, 3]), b
        assert not stats[b, g:].any(), b          # zeros for k >= gt_count[b]


_COMBOS = AC.combos()


@pytest.mark.parametrize("combo", _COMBOS, ids=[AC.combo_id(c) for c in _COMBOS])
def test_assignment_matches_reference(combo):
    case, kind, top_k = combo
    _check(case, kind, top_k, _generator(case, kind, top_k).from_boxes(case.boxes, return_matched=True, return_stats=True))


def _case(name):
    return next(c for c in AC.cases() if c.id == name)


def _staged(case):
    B, G = len(case.boxes), max([len(b) for b in case.boxes] + [1])
    gt = np.zeros((B, G, 7))
    for b, boxes in enumerate(case.boxes):
        gt[b, :len(boxes)] = boxes
    return B, case.n_anchors, G, torch.from_numpy(gt).to(DEV), torch.tensor([len(b) for b in case.boxes], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("kind", AC.KINDS)
def test_candidate_ious_are_vn_rpn_targets_iou_s(kind):
    """one box on 28 sites, top_k = 32: every anchor is a candidate, so mu is the mean of the IoU column vn_rpn_targets_iou
    computes — read from that call's workspace, whose first N doubles are m_n = IoU(n, 0) — added in the documented order
    (group 0 by rank, then group 1) and divided by 56: equal exactly; sd and t likewise up to the rounding of a square root"""
    from voxelnet_amd import _lib
    case = _case("Car-4x7-one-box")
    B, N, G, gt_d, cnt_d = _staged(case)
    assert (B, N, G) == (1, 56, 1)
    gen = _generator(case, kind, 32)
    stats = gen.from_boxes(case.boxes, return_stats=True)[3].cpu().numpy()[0, 0]
    nbytes = _lib.load().vn_rpn_targets_iou_workspace_bytes(B, N, G)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    outs = [torch.empty(N * k, dtype=torch.float32, device=DEV) for k in (1, 1, 7)]
    with _lib.on_device(torch.device(DEV)):
        _lib.call("vn_rpn_targets_iou", gen._anchors_dev.data_ptr(), N, gt_d.data_ptr(), cnt_d.data_ptr(), B, G, KIND_ID[kind],
                  0.6, 0.45, float(case.anchor_h), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None, ws.data_ptr(),
                  nbytes, _lib.raw_stream())
    torch.cuda.synchronize()
    col = ws[:N * 8].view(torch.float64).cpu().numpy()
    order = case.ref(kind, 32)[0]["cand"][0]
    assert np.array_equal(np.sort(order), np.arange(N)) and np.count_nonzero(col) >= 20
    total = 0.0
    for n in order:
        total += float(col[n])
    mu = total / N
    ss = 0.0
    for n in order:
        ss += (float(col[n]) - mu) * (float(col[n]) - mu)
    sd = float(np.sqrt(ss / (N - 1)))
    print(f"{kind}: mu {stats[0]!r} vs {mu!r}, sd {stats[1]!r} vs {sd!r}")
    assert stats[0] == mu
    np.testing.assert_allclose(stats[1:3], [sd, mu + sd], rtol=1e-15, atol=0)


@pytest.mark.parametrize("kind", AC.KINDS)
def test_deterministic_with_and_without_optional_outputs_and_inside_its_buffers(kind):
    """two calls bit-equal; matched / stats = NULL give the same maps; called directly on the 270-anchor grid with every output
    AND the workspace a view into a LARGER buffer pre-filled with a sentinel: what follows the bytes the call owns stays as it
    was; gt_count beyond [0, max_gt] is clamped"""
    from voxelnet_amd import _lib
    case = _case("Car-9x15")
    assert case.n_anchors == 270
    gen = _generator(case, kind, 9)
    first = gen.from_boxes(case.boxes, return_matched=True, return_stats=True)
    again = gen.from_boxes(case.boxes, return_matched=True, return_stats=True)
    three, four = gen.from_boxes(case.boxes), gen.from_boxes(case.boxes, return_stats=True)
    assert len(three) == 3 and len(four) == 4
    for x, y in zip(first, again):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for x, y in zip(first, three):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(first[4].view(torch.int32), four[3].view(torch.int32))
    B, N, G, gt_d, cnt_d = _staged(case)
    assert cnt_d.tolist() == [5, 0, 12] and G == 12
    gt_full = gt_d.clone()
    gt_full[0, 5:] = gt_d[2, 5:]          # valid boxes behind sample 0's count: they must not be read as boxes of sample 0
    SENTINEL, EXTRA = -7.0, 4096
    nbytes = _lib.load().vn_rpn_targets_atss_workspace_bytes(B, N, G, 9)
    assert nbytes > 0 and nbytes % 256 == 0
    for counts in ([5, 0, 12], [5, -3, 1000]):
        bufs = [torch.full((B * N * k + EXTRA,), SENTINEL, dtype=torch.float32, device=DEV) for k in (1, 1, 7)]
        mbuf = torch.full((B * N + EXTRA,), -7, dtype=torch.int32, device=DEV)
        sbuf = torch.full((B * G * 4 + EXTRA,), SENTINEL, dtype=torch.float64, device=DEV)
        ws = torch.full((nbytes + EXTRA,), 0xA5, dtype=torch.uint8, device=DEV)
        c_d = torch.tensor(counts, dtype=torch.int32, device=DEV)
        with _lib.on_device(torch.device(DEV)):
            _lib.call("vn_rpn_targets_atss", gen._anchors_dev.data_ptr(), N, gt_full.data_ptr(), c_d.data_ptr(), B, G, KIND_ID[kind],
                      9, float(case.anchor_h), bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), mbuf.data_ptr(),
                      sbuf.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
        torch.cuda.synchronize()
        for buf, k in zip(bufs, (1, 1, 7)):
            assert (buf[B * N * k:] == SENTINEL).all() and (buf[:B * N * k] != SENTINEL).all()
        assert (mbuf[B * N:] == -7).all() and (mbuf[:B * N] != -7).all()
        assert (sbuf[B * G * 4:] == SENTINEL).all() and (sbuf[:B * G * 4] != SENTINEL).all()
        assert (ws[nbytes:] == 0xA5).all()
        for buf, k, want in zip(bufs + [mbuf], (1, 1, 7, 1), first):
            assert torch.equal(buf[:B * N * k].view(torch.int32), want.reshape(-1).view(torch.int32))
        assert torch.equal(sbuf[:B * G * 4].view(torch.int64), first[4].reshape(-1).view(torch.int64))


def test_one_sample_and_an_empty_middle_sample():
    """B = 1 (128 boxes on 130 anchors: a grid of 128 x 1 workgroups) and B = 3 whose middle sample has no box"""
    one = _case("Car-5x13-128boxes")
    assert len(one.boxes) == 1 and len(one.boxes[0]) == 128
    pos, neg, _, matched, stats = _generator(one, "rotated", 9).from_boxes(one.boxes, return_matched=True, return_stats=True)
    ref = one.ref("rotated", 9)[0]
    assert np.array_equal(matched.cpu().numpy().reshape(-1), ref["matched"]) and stats.shape == (1, 128, 4)
    # B = 1 on the full grid, 12 boxes: the scan is cut into 64 chunks, its most — one per lane of the merging wave
    full = _case("Car-full")
    assert len(full.boxes[2]) == 12 and full.n_anchors == 70400
    for top_k in (9, 32):
        _, _, _, matched, stats = _generator(full, "rotated", top_k).from_boxes([full.boxes[2]], return_matched=True, return_stats=True)
        ref = full.ref("rotated", top_k)[2]
        assert np.array_equal(matched.cpu().numpy().reshape(-1), ref["matched"])
        assert np.array_equal(stats[0, :, 3].cpu().numpy(), ref["stats"][:, 3])
        assert float(np.abs(stats[0, :, :3].cpu().numpy() - ref["stats"][:, :3]).max()) <= 1e-9
    three = _case("Car-atss-extra")
    sub = [three.boxes[0], three.boxes[1], three.boxes[2]]
    assert [len(b) for b in sub] == [2, 0, 2]
    pos, neg, _, matched, stats = _generator(three, "standup", 9).from_boxes(sub, return_matched=True, return_stats=True)
    assert pos.shape[0] == 3 and not pos[1].any() and neg[1].all() and (matched[1] == -1).all() and not stats[1].any()
    for b in (0, 2):
        assert np.array_equal(matched[b].cpu().numpy().reshape(-1), three.ref("standup", 9)[b]["matched"])


def test_error_surface():
    from voxelnet_amd import _lib
    lib = _lib.load()
    case = _case("Car-5x13")
    B, N, G, gt_d, cnt_d = _staged(case)
    q = lib.vn_rpn_targets_atss_workspace_bytes
    nbytes = q(B, N, G, 9)
    assert nbytes > 0 and q(B, N, G, 1) > 0 and q(B, N, G, 32) > 0
    for bad in ((0, N, G, 9), (B, 0, G, 9), (B, N + 1, G, 9), (B, N, 0, 9), (B, N, 129, 9), (B, N, G, 0), (B, N, G, 33),
                (1 << 20, 1 << 10, G, 9)):
        assert q(*bad) == 0, bad
    a_d = torch.from_numpy(np.ascontiguousarray(case.anchors.reshape(-1, 7))).to(DEV)
    pos, neg = (torch.full((B * N,), -7.0, dtype=torch.float32, device=DEV) for _ in range(2))
    tgt = torch.full((B * N * 7,), -7.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    good = dict(anchors=a_d.data_ptr(), n=N, gt=gt_d.data_ptr(), cnt=cnt_d.data_ptr(), B=B, G=G, kind=2, top_k=9, h=1.56,
                pos=pos.data_ptr(), neg=neg.data_ptr(), tgt=tgt.data_ptr(), matched=None, stats=None, ws=ws.data_ptr(), nb=nbytes)

    def run(**kw):
        a = dict(good, **kw)
        with _lib.on_device(torch.device(DEV)):
            return lib.vn_rpn_targets_atss(a["anchors"], a["n"], a["gt"], a["cnt"], a["B"], a["G"], a["kind"], a["top_k"], a["h"],
                                           a["pos"], a["neg"], a["tgt"], a["matched"], a["stats"], a["ws"], a["nb"], _lib.raw_stream())
    for kw in (dict(anchors=None), dict(gt=None), dict(cnt=None), dict(pos=None), dict(neg=None), dict(tgt=None), dict(ws=None),
               dict(n=N + 1), dict(n=0), dict(B=0), dict(G=0), dict(G=129), dict(top_k=0), dict(top_k=33), dict(kind=0), dict(kind=3),
               dict(h=0.0)):
        assert run(**kw) == EINVAL, kw
    assert run(nb=nbytes - 1) == EWORKSPACE and run(nb=0) == EWORKSPACE
    torch.cuda.synchronize()
    assert (pos == -7).all() and (neg == -7).all() and (tgt == -7).all()          # nothing was launched
    assert run() == 0
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy().reshape(B, N), np.stack([s["pos"] for s in case.ref("rotated", 9)]).astype(np.float32))


def test_python_surface_and_anchor_mask():
    from voxelnet_amd import _lib
    from voxelnet_amd import targets as T
    case = _case("Car-9x15")
    for bad in (0, 33, -1, 2.5, True):
        with pytest.raises(ValueError):
            T.TargetGenerator("Car", DEV, anchors=case.anchors, assign="atss", atss_top_k=bad)
    with pytest.raises(ValueError):
        T.TargetGenerator("Car", DEV, anchors=case.anchors, assign="atss", atss_iou="reference")
    with pytest.raises(_lib.VoxelnetHipError):
        T.TargetGenerator("Car", "cpu", assign="atss")
    for other in ("reference", "standup", "rotated"):
        with pytest.raises(ValueError):
            T.TargetGenerator("Car", DEV, anchors=case.anchors, assign=other).from_boxes(case.boxes, return_stats=True)
    with pytest.raises(_lib.VoxelnetHipError):
        _generator(case, "rotated", 9).from_boxes([np.zeros((129, 7))])
    assert T.ASSIGN_KINDS["atss"] is None and "atss" in T.ASSIGN_KINDS
    # pos_iou / neg_iou are accepted and ignored
    gen, odd = _generator(case, "rotated", 9), _generator(case, "rotated", 9, pos_iou=0.99, neg_iou=0.01)
    plain = gen.from_boxes(case.boxes, return_matched=True, return_stats=True)
    for x, y in zip(plain, odd.from_boxes(case.boxes, return_matched=True, return_stats=True)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # anchor_mask= composes: an anchor the mask leaves out is ignored (pos = neg = 0), every other entry and the rest unchanged
    rng = np.random.default_rng(11)
    mask = torch.from_numpy((rng.random(tuple(plain[0].shape)) < 0.5).astype(np.uint8)).to(DEV)
    masked = gen.from_boxes(case.boxes, return_matched=True, return_stats=True, anchor_mask=mask)
    keep = mask.bool()
    assert int((plain[0].bool() & ~keep).sum()) > 0          # the mask does hide positives
    assert torch.equal(masked[0], plain[0] * keep) and torch.equal(masked[1], plain[1] * keep)
    for x, y in zip(plain[2:], masked[2:]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- the model
def _tiny_model(top_k=9, kind="rotated", mode="bf16", **kw):
    from voxelnet_amd import model as M
    from voxelnet_amd.targets import TargetGenerator
    M.set_precision(mode)
    torch.manual_seed(7)
    m = M.RPN3D("Car", cls_loss="focal", yaw_loss="sin", target_assign="atss", atss_top_k=top_k, atss_iou=kind, **kw)
    res = m.load_state_dict(tr.make_state_dict("Car"), strict=False)
    assert all("dir_conv" in k or "iou_conv" in k for k in res.missing_keys) and not res.unexpected_keys
    m.feature_net._grid = replace(m.feature_net._grid, H=16, W=24)
    m = m.to(DEV).train()
    # the module's generator on the tiny grid's anchors (its own is the full 200 x 176 grid's)
    m.__dict__["_targets"] = TargetGenerator("Car", torch.device(DEV), anchors=GA._tiny_anchors(), assign="atss", atss_top_k=top_k,
                                             atss_iou=kind, keep_heading=bool(kw.get("dir_head")))
    return m


def test_rpn3d_reaches_the_generator_and_rebuilds_on_change():
    from voxelnet_amd import model as M
    from voxelnet_amd import targets as T
    labels = [AC.C.round_trip_frames(T.generate_anchors("Car"))[0]]
    for kw in (dict(atss_top_k=0), dict(atss_top_k=33), dict(atss_iou="iou")):
        with pytest.raises(ValueError):
            M.RPN3D("Car", target_assign="atss", **kw)
    assert (M.RPN3D("Car").atss_top_k, M.RPN3D("Car").atss_iou) == (9, "rotated")
    m = M.RPN3D("Car", target_assign="atss", atss_top_k=12, atss_iou="standup")
    dev = torch.device(DEV)
    gen = m._target_generator(dev)
    assert (gen.assign, gen.atss_top_k, gen.atss_iou) == ("atss", 12, "standup") and gen is m._target_generator(dev)
    assert tuple(gen.shape) == (200, 176)
    own = gen(labels)
    alone = T.TargetGenerator("Car", DEV, assign="atss", atss_top_k=12, atss_iou="standup")(labels)
    rotated = T.TargetGenerator("Car", DEV, assign="rotated")(labels)
    for x, y in zip(own, alone):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert int(own[0].sum()) >= 2 and not torch.equal(own[0], rotated[0])
    assert torch.equal(own[1], 1 - own[0])          # no ignore band
    m.atss_top_k = 5          # set after construction: the next call rebuilds the generator
    g5 = m._target_generator(dev)
    assert g5 is not gen and g5.atss_top_k == 5 and g5.atss_iou == "standup"
    m.atss_iou = "rotated"
    g6 = m._target_generator(dev)
    assert g6 is not g5 and (g6.atss_top_k, g6.atss_iou) == (5, "rotated") and g6 is m._target_generator(dev)
    m.target_assign = "rotated"
    assert m._target_generator(dev).assign == "rotated"


@pytest.mark.parametrize("heads", [dict(), dict(dir_head=True, iou_head=True)], ids=["plain", "dir+iou"])
def test_train_step_with_atss_assignment(golden, heads):
    """the tiny golden batch with labels, target_assign="atss": RPN3D.train_step generating its targets itself equals a
    train_step handed the generator's maps precomputed — the outputs, every .grad and every updated weight bit for bit — and
    differs from the rotated assignment's step.  Without heads it is the ONE fused call; with the direction and IoU heads (the
    consumers of the positives' boxes) it takes the separate calls."""
    from voxelnet_amd import model as M
    from voxelnet_amd.optim import ClipSGD
    feats, coords = GA._tiny(golden)
    labels = GA._tiny_labels()
    batch = (None, labels, feats, None, coords, None, None)
    dev = torch.device(DEV)
    try:
        a = _tiny_model(**heads)
        assert a._step_fused_ok("bf16", None) == (not heads)
        oa = ClipSGD(a.parameters(), lr=1e-3, max_norm=5.0)
        out_a = a.train_step(batch, DEV, oa)
        b = _tiny_model(**heads)
        want = b._target_generator(dev)(labels)
        ob = ClipSGD(b.parameters(), lr=1e-3, max_norm=5.0)
        out_b = b.train_step(batch, DEV, ob, targets=want)
        c = _tiny_model(**heads)
        c.target_assign = "rotated"
        c.__dict__.pop("_targets")
        from voxelnet_amd.targets import TargetGenerator
        c.__dict__["_targets"] = TargetGenerator("Car", dev, anchors=GA._tiny_anchors(), assign="rotated",
                                                 keep_heading=bool(heads.get("dir_head")))
        out_c = c.train_step(batch, DEV, None)
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    gen = a._target_generator(dev)
    assert gen.assign == "atss" and tuple(gen.shape) == (8, 12) and int(want[0].sum()) >= 3
    assert len(out_a) == len(out_b) == 7
    for i, (x, y) in enumerate(zip(out_a, out_b)):
        assert torch.isfinite(x).all() and torch.equal(x, y), ("output", i)
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    init = tr.make_state_dict("Car")
    for k in pa:
        assert pa[k].grad is not None and torch.isfinite(pa[k].grad).all() and torch.equal(pa[k].grad, pb[k].grad), k
        assert torch.equal(pa[k].detach(), pb[k].detach()), k
    k = "middle_rpn.block3.0.conv.weight"
    assert not torch.equal(pa[k].detach().cpu(), init[k])          # the weights did move
    assert torch.equal(out_a[0], out_c[0]) and float(out_a[2].detach()) != float(out_c[2].detach())         # same maps, other targets
    if heads:
        assert float(a.last_dir[0]) > 0 and float(a.last_iou_head[0]) > 0
