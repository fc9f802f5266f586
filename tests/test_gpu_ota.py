"""GPU: the SimOTA target assignment (csrc/targets_ota.hip through vn_rpn_targets_ota / targets.TargetGenerator(assign="simota") /
RPN3D(target_assign="simota")) against the restatement tests/ota_ref.py.

Bars.  The guard is asserted ON THE REFERENCE ALONE first (ota_cases.MARGIN = 1e-6): no footprint edge, radius, floor of sum_k,
selection cut or two-box tie within the margin, and every candidate's IoU exactly 0 or >= 1e-4.  Then pos, neg, targets,
matched and the stats' counts and dyn_k must be equal exactly, sum_k within 1e-9 (DESIGN.md 1o measured <= 8e-16 for the same
pair function) and the cut cost within 1e-7 (with v = 0 or >= 1e-4 a v error of 1e-13 moves a cost by at most 3e-9).

Shapes (tests/ota_cases.py): 2, 130, 270, 810 (tiled: copies), 1,536 and 70,400 anchors, Pedestrian anchors, 128 boxes on 130
anchors, frames with copies / an invalid box / a box off the grid / an empty sample, zero deltas with one p, p = 0, p = NaN, an
overflowing delta, one box whose candidates all score 0.8, radius 0, a radius wider than the grid with the scan in ONE chunk
(24 candidates per lane: the bounded lists overflow); q 1, 10, 16 (and 7); both metrics."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import ota_cases as OC
import test_gpu_assign as GA
from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
METRIC_ID = {"bev": 0, "3d": 1}
EINVAL, EWORKSPACE = -1, -3


def _generator(case, metric, q, **kw):
    from voxelnet_amd import targets as T
    return T.TargetGenerator(case.cls_name, DEV, anchors=case.anchors, assign="simota", ota_q=q, ota_radius=case.radius,
                             ota_iou_weight=case.iou_weight, ota_metric=metric, **kw)


def _maps(case):
    return dict(probs=torch.tensor(case.probs, device=DEV), deltas=torch.tensor(case.deltas, device=DEV))


def _check(case, metric, q, out):
    gaps = case.guard(metric, q)          # on the reference alone, before the device is looked at
    print(f"{case.id} {metric} q {q}: smallest gaps of the reference's decisions {gaps}")
    assert all(g > OC.MARGIN for g in gaps.values())
    pos, neg, tgt, matched, stats = (t.cpu().numpy() for t in out)
    B, N, G = len(case.boxes), case.n_anchors, max([len(b) for b in case.boxes] + [1])
    assert pos.shape == (B, *case.shape, 2) and neg.shape == pos.shape and matched.shape == pos.shape
    assert tgt.shape == (B, *case.shape, 14) and stats.shape == (B, G, 5)
    assert pos.dtype == np.float32 and neg.dtype == np.float32 and tgt.dtype == np.float32
    assert matched.dtype == np.int32 and stats.dtype == np.float64
    for b, ref in enumerate(case.ref(metric, q)):
        g = ref["stats"].shape[0]
        e_sum = float(np.abs(stats[b, :g, 1] - ref["stats"][:, 1]).max()) if g else 0.0
        e_cut = float(np.abs(stats[b, :g, 3] - ref["stats"][:, 3]).max()) if g else 0.0
        t, r = tgt[b].reshape(N, 7), ref["targets"]
        print(f"  sample {b}: {int(ref['pos'].sum())} positives, sum_k error {e_sum:.2e}, cut cost error {e_cut:.2e}, "
              f"targets differ in {int((t != r).sum())} elements")
        assert np.array_equal(stats[b, :g][:, [0, 2]], ref["stats"][:, [0, 2]]), b
        assert np.array_equal(matched[b].reshape(N), ref["matched"]), b
        assert np.array_equal(pos[b].reshape(N), ref["pos"].astype(np.float32)), b
        assert np.array_equal(neg[b].reshape(N), ref["neg"].astype(np.float32)), b
        assert np.array_equal(t, r), b
        assert e_sum <= 1e-9 and e_cut <= 1e-7, (b, e_sum, e_cut)
        assert np.array_equal(stats[b, :g, 4], ref["stats"][:, 4]), b
        assert not stats[b, g:].any(), b          # zeros for k >= gt_count[b]


_COMBOS = OC.combos()


@pytest.mark.parametrize("combo", _COMBOS, ids=[OC.combo_id(c) for c in _COMBOS])
def test_assignment_matches_reference(combo):
    case, metric, q = combo
    _check(case, metric, q, _generator(case, metric, q).from_boxes(case.boxes, return_matched=True, return_stats=True, **_maps(case)))


def _case(name):
    return next(c for c in OC.cases() if c.id == name)


def _staged(case):
    B, G = len(case.boxes), max([len(b) for b in case.boxes] + [1])
    gt = np.zeros((B, G, 7))
    for b, boxes in enumerate(case.boxes):
        gt[b, :len(boxes)] = boxes
    return B, case.n_anchors, G, torch.from_numpy(gt).to(DEV), torch.tensor([len(b) for b in case.boxes], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("metric", OC.METRICS)
def test_deterministic_with_and_without_optional_outputs_and_inside_its_buffers(metric):
    """two calls bit-equal; matched / stats = NULL give the same maps; called directly on the 270-anchor grid with every output
    AND the workspace a view into a LARGER buffer pre-filled with a sentinel: what follows the bytes the call owns stays as it
    was; gt_count beyond [0, max_gt] is clamped"""
    from voxelnet_amd import _lib
    case = _case("Car-9x15")
    assert case.n_anchors == 270
    gen, maps = _generator(case, metric, 10), _maps(case)
    first = gen.from_boxes(case.boxes, return_matched=True, return_stats=True, **maps)
    again = gen.from_boxes(case.boxes, return_matched=True, return_stats=True, **maps)
    three, four = gen.from_boxes(case.boxes, **maps), gen.from_boxes(case.boxes, return_stats=True, **maps)
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
    nbytes = _lib.load().vn_rpn_targets_ota_workspace_bytes(B, N, G, 10)
    assert nbytes > 0 and nbytes % 256 == 0
    for counts in ([5, 0, 12], [5, -3, 1000]):
        bufs = [torch.full((B * N * k + EXTRA,), SENTINEL, dtype=torch.float32, device=DEV) for k in (1, 1, 7)]
        mbuf = torch.full((B * N + EXTRA,), -7, dtype=torch.int32, device=DEV)
        sbuf = torch.full((B * G * 5 + EXTRA,), SENTINEL, dtype=torch.float64, device=DEV)
        ws = torch.full((nbytes + EXTRA,), 0xA5, dtype=torch.uint8, device=DEV)
        c_d = torch.tensor(counts, dtype=torch.int32, device=DEV)
        with _lib.on_device(torch.device(DEV)):
            _lib.call("vn_rpn_targets_ota", gen._anchors_dev.data_ptr(), N, gt_full.data_ptr(), c_d.data_ptr(), B, G,
                      maps["probs"].data_ptr(), maps["deltas"].data_ptr(), METRIC_ID[metric], 10, case.radius, case.iou_weight,
                      float(case.anchor_h), bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), mbuf.data_ptr(),
                      sbuf.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
        torch.cuda.synchronize()
        for buf, k in zip(bufs, (1, 1, 7)):
            assert (buf[B * N * k:] == SENTINEL).all() and (buf[:B * N * k] != SENTINEL).all()
        assert (mbuf[B * N:] == -7).all() and (mbuf[:B * N] != -7).all()
        assert (sbuf[B * G * 5:] == SENTINEL).all() and (sbuf[:B * G * 5] != SENTINEL).all()
        assert (ws[nbytes:] == 0xA5).all()
        for buf, k, want in zip(bufs + [mbuf], (1, 1, 7, 1), first):
            assert torch.equal(buf[:B * N * k].view(torch.int32), want.reshape(-1).view(torch.int32))
        assert torch.equal(sbuf[:B * G * 5].view(torch.int64), first[4].reshape(-1).view(torch.int64))


def test_error_surface():
    from voxelnet_amd import _lib
    lib = _lib.load()
    case = _case("Car-5x13")
    B, N, G, gt_d, cnt_d = _staged(case)
    q = lib.vn_rpn_targets_ota_workspace_bytes
    nbytes = q(B, N, G, 10)
    assert nbytes > 0 and q(B, N, G, 1) > 0 and q(B, N, G, 16) > 0
    for bad in ((0, N, G, 10), (B, 0, G, 10), (B, N + 1, G, 10), (B, N, 0, 10), (B, N, 129, 10), (B, N, G, 0), (B, N, G, 17),
                (1 << 20, 1 << 10, G, 10)):
        assert q(*bad) == 0, bad
    a_d = torch.from_numpy(np.ascontiguousarray(case.anchors.reshape(-1, 7))).to(DEV)
    maps = _maps(case)
    pos, neg = (torch.full((B * N,), -7.0, dtype=torch.float32, device=DEV) for _ in range(2))
    tgt = torch.full((B * N * 7,), -7.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    good = dict(anchors=a_d.data_ptr(), n=N, gt=gt_d.data_ptr(), cnt=cnt_d.data_ptr(), B=B, G=G, probs=maps["probs"].data_ptr(),
                deltas=maps["deltas"].data_ptr(), metric=0, q=10, radius=case.radius, w=3.0, h=1.56, pos=pos.data_ptr(),
                neg=neg.data_ptr(), tgt=tgt.data_ptr(), matched=None, stats=None, ws=ws.data_ptr(), nb=nbytes)

    def run(**kw):
        a = dict(good, **kw)
        with _lib.on_device(torch.device(DEV)):
            return lib.vn_rpn_targets_ota(a["anchors"], a["n"], a["gt"], a["cnt"], a["B"], a["G"], a["probs"], a["deltas"], a["metric"],
                                          a["q"], a["radius"], a["w"], a["h"], a["pos"], a["neg"], a["tgt"], a["matched"], a["stats"],
                                          a["ws"], a["nb"], _lib.raw_stream())
    inf, nan = float("inf"), float("nan")
    for kw in (dict(anchors=None), dict(gt=None), dict(cnt=None), dict(probs=None), dict(deltas=None), dict(pos=None), dict(neg=None),
               dict(tgt=None), dict(ws=None), dict(n=N + 1), dict(n=0), dict(B=0), dict(G=0), dict(G=129), dict(q=0), dict(q=17),
               dict(metric=-1), dict(metric=2), dict(radius=-0.5), dict(radius=nan), dict(radius=inf), dict(w=-1.0), dict(w=nan),
               dict(w=inf), dict(h=0.0)):
        assert run(**kw) == EINVAL, kw
    assert run(nb=nbytes - 1) == EWORKSPACE and run(nb=0) == EWORKSPACE
    torch.cuda.synchronize()
    assert (pos == -7).all() and (neg == -7).all() and (tgt == -7).all()          # nothing was launched
    assert run() == 0 and run(radius=0.0) == 0 and run(w=0.0) == 0
    assert run() == 0
    torch.cuda.synchronize()
    assert np.array_equal(pos.cpu().numpy().reshape(B, N), np.stack([s["pos"] for s in case.ref("bev", 10)]).astype(np.float32))


def test_python_surface_and_anchor_mask():
    from voxelnet_amd import _lib
    from voxelnet_amd import targets as T
    case = _case("Car-9x15")
    maps = _maps(case)
    gen = _generator(case, "bev", 10)
    with pytest.raises(_lib.VoxelnetHipError):
        T.TargetGenerator("Car", "cpu", assign="simota")
    # the maps: required under "simota", refused under every other kind, and of the generator's grid
    for kw in (dict(), dict(probs=maps["probs"]), dict(deltas=maps["deltas"]), dict(probs=maps["probs"][:2], deltas=maps["deltas"]),
               dict(probs=maps["probs"], deltas=maps["deltas"][:, :, :8]), dict(probs=maps["probs"].double(), deltas=maps["deltas"]),
               dict(probs=maps["probs"].cpu(), deltas=maps["deltas"].cpu())):
        with pytest.raises(ValueError):
            gen.from_boxes(case.boxes, **kw)
    for other in ("reference", "standup", "rotated", "atss"):
        with pytest.raises(ValueError):
            T.TargetGenerator("Car", DEV, anchors=case.anchors, assign=other).from_boxes(case.boxes, **maps)
    with pytest.raises(ValueError):
        T.TargetGenerator("Car", DEV, anchors=case.anchors, assign="rotated").from_boxes(case.boxes, return_stats=True)
    with pytest.raises(_lib.VoxelnetHipError):
        gen.from_boxes([np.zeros((129, 7))], probs=maps["probs"][:1], deltas=maps["deltas"][:1])
    # ota_radius=None: 2.5 site pitches, read from the anchors
    auto = T.TargetGenerator("Car", DEV, anchors=case.anchors, assign="simota")
    assert auto.ota_radius == case.radius == 2.5 * T.site_pitch(case.anchors) and (auto.ota_q, auto.ota_iou_weight, auto.ota_metric) == (10, 3.0, "bev")
    plain = gen.from_boxes(case.boxes, return_matched=True, return_stats=True, **maps)
    for x, y in zip(plain, auto.from_boxes(case.boxes, return_matched=True, return_stats=True, **maps)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # non-contiguous maps are read as their values
    wide = torch.zeros((3, 2, 9, 30), device=DEV)
    wide[..., ::2] = maps["probs"]
    for x, y in zip(plain, gen.from_boxes(case.boxes, return_matched=True, return_stats=True, probs=wide[..., ::2], deltas=maps["deltas"])):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    # anchor_mask= composes: an anchor the mask leaves out is ignored (pos = neg = 0), every other entry and the rest unchanged
    rng = np.random.default_rng(11)
    mask = torch.from_numpy((rng.random(tuple(plain[0].shape)) < 0.5).astype(np.uint8)).to(DEV)
    masked = gen.from_boxes(case.boxes, return_matched=True, return_stats=True, anchor_mask=mask, **maps)
    keep = mask.bool()
    assert int((plain[0].bool() & ~keep).sum()) > 0          # the mask does hide positives
    assert torch.equal(masked[0], plain[0] * keep) and torch.equal(masked[1], plain[1] * keep)
    for x, y in zip(plain[2:], masked[2:]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- the model
def _tiny_model(mode="bf16", **kw):
    from voxelnet_amd import model as M
    from voxelnet_amd.targets import TargetGenerator
    M.set_precision(mode)
    torch.manual_seed(7)
    m = M.RPN3D("Car", cls_loss="focal", yaw_loss="sin", target_assign="simota", **kw)
    res = m.load_state_dict(tr.make_state_dict("Car"), strict=False)
    assert all("dir_conv" in k or "iou_conv" in k for k in res.missing_keys) and not res.unexpected_keys
    m.feature_net._grid = replace(m.feature_net._grid, H=16, W=24)
    m = m.to(DEV).train()
    # the module's generator on the tiny grid's anchors (its own is the full 200 x 176 grid's)
    m.__dict__["_targets"] = TargetGenerator("Car", torch.device(DEV), anchors=GA._tiny_anchors(), assign="simota",
                                             keep_heading=bool(kw.get("dir_head")))
    return m


def test_rpn3d_reaches_the_generator_and_rebuilds_on_change():
    from voxelnet_amd import model as M
    for kw in (dict(ota_q=0), dict(ota_q=17), dict(ota_radius=-1.0), dict(ota_iou_weight=float("nan")), dict(ota_metric="rotated")):
        with pytest.raises(ValueError):
            M.RPN3D("Car", target_assign="simota", **kw)
    d = M.RPN3D("Car")
    assert (d.target_assign, d.ota_q, d.ota_radius, d.ota_iou_weight, d.ota_metric) == ("reference", 10, None, 3.0, "bev")
    m = M.RPN3D("Car", target_assign="simota", ota_q=7, ota_radius=1.5, ota_iou_weight=2.0, ota_metric="3d")
    dev = torch.device(DEV)
    gen = m._target_generator(dev)
    assert (gen.assign, gen.ota_q, gen.ota_radius, gen.ota_iou_weight, gen.ota_metric) == ("simota", 7, 1.5, 2.0, "3d")
    assert gen is m._target_generator(dev) and tuple(gen.shape) == (200, 176)
    m.ota_q = 5          # set after construction: the next call rebuilds the generator
    g5 = m._target_generator(dev)
    assert g5 is not gen and g5.ota_q == 5 and g5.ota_metric == "3d"
    m.ota_radius = None
    g6 = m._target_generator(dev)
    assert g6 is not g5 and 1.00 < g6.ota_radius < 1.01 and g6 is m._target_generator(dev)          # 2.5 x 0.4023 m
    m.target_assign = "atss"
    assert m._target_generator(dev).assign == "atss"


@pytest.mark.parametrize("heads", [dict(), dict(dir_head=True, iou_head=True)], ids=["plain", "dir+iou"])
def test_forward_and_train_step_with_simota_assignment(golden, heads):
    """the tiny golden batch with labels, target_assign="simota".  forward() generating its targets itself, after detect() and
    from its own maps, equals forward(targets=) handed the generator's maps of a first forward's predictions, bit for bit.
    train_step() — the separate calls: the one call cannot hand out the maps between its forward and its loss — equals forward +
    backward + step: the outputs, every .grad and every updated weight bit for bit.  train_step(targets=) still takes the ONE
    call (without heads), and forward() is never entered."""
    from voxelnet_amd import model as M
    from voxelnet_amd.optim import ClipSGD
    feats, coords = GA._tiny(golden)
    labels = GA._tiny_labels()
    batch = (None, labels, feats, None, coords, None, None)
    dev = torch.device(DEV)
    try:
        f = _tiny_model(**heads)
        own = f(batch, DEV)
        want = f._target_generator(dev)(labels, probs=own[0].detach(), deltas=own[1].detach())
        handed = f(batch, DEV, targets=want)
        a = _tiny_model(**heads)
        assert not a._step_fused_ok("bf16", None) and a._step_fused_ok("bf16", None, want) == (not heads)
        oa = ClipSGD(a.parameters(), lr=1e-3, max_norm=5.0)
        out_a = a.train_step(batch, DEV, oa)
        b = _tiny_model(**heads)
        ob = ClipSGD(b.parameters(), lr=1e-3, max_norm=5.0)
        out_b = b(batch, DEV)
        out_b[2].backward()
        ob.step()
        out_c = None
        if not heads:
            c = _tiny_model()
            oc = ClipSGD(c.parameters(), lr=1e-3, max_norm=5.0)

            def no_forward(*args, **kw):
                raise AssertionError("train_step(targets=) entered forward(): not the one-call step")
            c.forward = no_forward
            out_c = c.train_step(batch, DEV, oc, targets=want)
        torch.cuda.synchronize()
    finally:
        M.set_precision("bf16")
    gen = f._target_generator(dev)
    assert gen.assign == "simota" and tuple(gen.shape) == (8, 12) and int(want[0].sum()) >= 3
    assert torch.equal(want[1], 1 - want[0])
    assert len(own) == len(handed) == len(out_a) == len(out_b) == 7
    for i, (x, y) in enumerate(zip(own, handed)):
        assert torch.isfinite(x).all() and torch.equal(x, y), ("forward output", i)
    others = [(out_b, b)] + ([(out_c, c)] if out_c is not None else [])
    pa = dict(a.named_parameters())
    init = tr.make_state_dict("Car")
    for out_o, o in others:
        for i, (x, y) in enumerate(zip(out_a, out_o)):
            assert torch.isfinite(x).all() and torch.equal(x, y), ("output", i)
        po = dict(o.named_parameters())
        for k in pa:
            assert pa[k].grad is not None and torch.isfinite(pa[k].grad).all() and torch.equal(pa[k].grad, po[k].grad), k
            assert torch.equal(pa[k].detach(), po[k].detach()), k
    for i, (x, y) in enumerate(zip(own, out_a)):
        assert torch.equal(x.detach(), y.detach()), ("forward vs train_step output", i)
    k = "middle_rpn.block3.0.conv.weight"
    assert not torch.equal(pa[k].detach().cpu(), init[k])          # the weights did move
    if heads:
        assert float(a.last_dir[0]) > 0 and float(a.last_iou_head[0]) > 0
