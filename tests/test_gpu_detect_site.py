"""GPU: the detection tail in the layout the loss trains (csrc/detect.hip's VN_DETECT_SITE through
vn_rpn_select_decode_layout / vn_rpn_detect_layout and predict.BoxDecoder(layout=)), and the round trip that pins the
true-IoU target assignment (csrc/targets_iou.hip) and that tail to the loss's layout.

Bars.  layout="site" on (probs, deltas) against the existing flat entry points on contiguous channels-last copies
probs.permute(0,2,3,1), deltas.permute(0,2,3,1): counts, scores, indices and boxes bit-identical.  Against
tests/detect_ref.py fed the channels-last copies, that file's bars (tests/test_gpu_detect.py): indices and scores bit-exact,
boxes rtol 2.4e-7, atol 1e-6.  VN_DETECT_FLAT through the new symbols against the old symbols: bit-identical.

The round trip is a condition, not a measurement: maps of a "perfect network" built from the assigner's own pos / targets,
decoded with predict.TRAINED_DECODE and scored by evaluate.DetectionEvaluator, must give BEV and 3D AP = 1.0 at every
difficulty and exactly one detection per ground truth, for both kinds (the CPU references alone meet it: DESIGN.md 1h)."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import assign_cases as C
import detect_ref as D
import test_gpu_detect as G
from oracle import targets as ot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SCENES = ("dense", "spread", "ped")
SEEDS = G.SEEDS          # (5, 6)
MODES = G.MODES


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _channels_last(t):
    """(B,C,h,w) -> a contiguous tensor whose flat memory is the (B,h,w,C) order, reshaped back to (B,C,h,w) sizes: what the
    flat layout reads as candidate j = (iy*W + ix)*2 + a"""
    return t.permute(0, 2, 3, 1).contiguous().view(t.shape)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------ 1. site == flat on channels-last
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("scene", SCENES)
def test_site_candidates_are_the_flat_candidates_of_the_channels_last_maps(scene, seed):
    probs, deltas = G._maps(scene, seed)
    _, thres, pre = G.SCENES[scene]
    dec = G._decoder(scene)
    p, d = _dev(probs), _dev(deltas)
    pc, dc = _channels_last(p), _channels_last(d)
    site = dec.candidates_device(p, d, thres, pre, layout="site")
    flat = dec.candidates_device(pc, dc, thres, pre)
    assert int(site[3].min()) == pre                                  # the cut truncates, as in tests/test_gpu_detect.py
    for x, y in zip(site, flat):
        assert torch.equal(_bits(x), _bits(y))
    assert not torch.equal(site[2], dec.candidates_device(p, d, thres, pre)[2])          # and it is another reading of the maps
    # against the reference fed the channels-last copies
    got = tuple(t.cpu().numpy() for t in site)
    G._check_selection(pc.cpu().numpy(), dc.cpu().numpy(), G._anchors(scene), thres, pre, got, G.SCENE_CLASS.get(scene, "Car"))
    # sel_idx is the anchor index n = 2 * site + rotation: the score came from probs[b, a, site]
    B, N = probs.shape[0], dec.n_anchors
    pf = probs.reshape(B, 2, N // 2)
    for b in range(B):
        n = got[2][b].astype(np.int64)
        assert np.array_equal(G._u32(got[1][b]), G._u32(pf[b, n & 1, n >> 1]))


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("scene", SCENES)
def test_site_detect_is_the_flat_detect_of_the_channels_last_maps(scene, seed, mode):
    probs, deltas = G._maps(scene, seed)
    _, thres, pre = G.SCENES[scene]
    dec = G._decoder(scene)
    p, d = _dev(probs), _dev(deltas)
    pc, dc = _channels_last(p), _channels_last(d)
    for thr, post in ((0.1, 64), (0.5, 20)):
        site = dec.decode_device(p, d, thres, thr, post, nms=mode, pre_nms_top_k=pre, layout="site")
        flat = dec.decode_device(pc, dc, thres, thr, post, nms=mode, pre_nms_top_k=pre)
        assert int(site[2].min()) > 0
        for x, y in zip(site, flat):
            assert torch.equal(_bits(x), _bits(y))
        again = dec.decode_device(p, d, thres, thr, post, nms=mode, pre_nms_top_k=pre, layout="site")
        for x, y in zip(site, again):
            assert torch.equal(_bits(x), _bits(y))
    if mode == "standup":
        # the reference's tail (pre_nms_top_k None) in the site layout: vn_rpn_predict on the channels-last copies
        st = 0.96 if scene == "ped" else 0.9
        site = dec.decode_device(p, d, st, 0.1, 20, layout="site")
        flat = dec.decode_device(pc, dc, st, 0.1, 20)
        assert int(site[2].sum()) > 0
        for x, y in zip(site, flat):
            assert torch.equal(_bits(x), _bits(y))


def test_site_detect_matches_reference_end_to_end():
    """the whole chain against detect_ref.detect fed the channels-last copies, on the spread scene (as
    tests/test_gpu_detect.py::test_detect_matches_reference_end_to_end): same detections; a decoder built with layout="site"
    takes it as its default, and __call__ passes layout on"""
    from voxelnet_amd.predict import BoxDecoder
    probs, deltas = G._maps("spread", 5)
    _, thres, pre = G.SCENES["spread"]
    pc = np.ascontiguousarray(probs.transpose(0, 2, 3, 1))
    dc = np.ascontiguousarray(deltas.transpose(0, 2, 3, 1))
    own = BoxDecoder("Car", DEV, anchors=G._anchors("spread"), layout="site")
    for mode in sorted(MODES):
        boxes, scores = G._decoder("spread")(_dev(probs), _dev(deltas), thres, 0.1, 20, nms=mode, pre_nms_top_k=pre, layout="site")
        b2, s2 = own(_dev(probs), _dev(deltas), thres, 0.1, 20, nms=mode, pre_nms_top_k=pre)
        for b in range(2):
            rb, rs = D.detect(pc[b], dc[b], G._anchors("spread"), thres, pre, MODES[mode], 0.1, 20)
            assert np.array_equal(G._u32(scores[b]), G._u32(rs)), (mode, b)
            np.testing.assert_allclose(boxes[b], rb, rtol=2.4e-7, atol=1e-6)
            assert np.array_equal(G._u32(boxes[b]), G._u32(b2[b])) and np.array_equal(G._u32(scores[b]), G._u32(s2[b]))


# ------------------------------------------------------------------------------ 2. VN_DETECT_FLAT == the old symbols
@pytest.mark.parametrize("scene", SCENES)
def test_flat_through_the_new_symbols_is_the_old_symbols(scene):
    from voxelnet_amd import _lib
    probs, deltas = G._maps(scene, 6)
    _, thres, pre = G.SCENES[scene]
    dec = G._decoder(scene)
    p, d = _dev(probs), _dev(deltas)
    B, N = 2, dec.n_anchors
    lib = _lib.load()
    old = dec.candidates_device(p, d, thres, pre)
    boxes = torch.zeros((B, pre, 7), dtype=torch.float32, device=DEV)
    scores = torch.zeros((B, pre), dtype=torch.float32, device=DEV)
    idx = torch.zeros((B, pre), dtype=torch.int32, device=DEV)
    counts = torch.zeros(B, dtype=torch.int32, device=DEV)
    nbytes = lib.vn_rpn_select_decode_workspace_bytes(B, N, pre)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.call("vn_rpn_select_decode_layout", p.data_ptr(), d.data_ptr(), dec._anchors_dev.data_ptr(), B, N, float(thres), pre,
              dec.anchor_h, boxes.data_ptr(), scores.data_ptr(), idx.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes,
              _lib.raw_stream(), _lib.VN_DETECT_FLAT)
    for x, y in zip(old, (boxes, scores, idx, counts)):
        assert torch.equal(_bits(x), _bits(y))
    for mode in sorted(MODES):
        old = dec.decode_device(p, d, thres, 0.1, 20, nms=mode, pre_nms_top_k=pre)
        ob = torch.zeros((B, 20, 7), dtype=torch.float32, device=DEV)
        os_ = torch.zeros((B, 20), dtype=torch.float32, device=DEV)
        oc = torch.zeros(B, dtype=torch.int32, device=DEV)
        nbytes = lib.vn_rpn_detect_workspace_bytes(B, N, pre)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.call("vn_rpn_detect_layout", p.data_ptr(), d.data_ptr(), dec._anchors_dev.data_ptr(), B, N, float(thres), pre,
                  MODES[mode], 0.1, 20, dec.anchor_h, ob.data_ptr(), os_.data_ptr(), oc.data_ptr(), ws.data_ptr(), nbytes,
                  _lib.raw_stream(), _lib.VN_DETECT_FLAT)
        assert int(oc.sum()) > 0
        for x, y in zip(old, (ob, os_, oc)):
            assert torch.equal(_bits(x), _bits(y))


def test_site_layout_argument_errors():
    from voxelnet_amd import _lib
    from voxelnet_amd.predict import TRAINED_DECODE, EVAL_DECODE, BoxDecoder
    assert TRAINED_DECODE == dict(EVAL_DECODE, layout="site") and "layout" not in EVAL_DECODE
    probs, deltas = G._maps("dense", 5)
    dec = G._decoder("dense")
    p, d = _dev(probs), _dev(deltas)
    with pytest.raises(ValueError):
        dec.decode_device(p, d, layout="nhwc")
    with pytest.raises(ValueError):
        dec.candidates_device(p, d, 0.5, 64, layout="nhwc")
    with pytest.raises(ValueError):
        BoxDecoder("Car", DEV, layout="nhwc")
    with pytest.raises(_lib.VoxelnetHipError):
        dec.decode_device(p.cpu(), d, layout="site")
    # an odd anchor count has no (site, rotation) reading: VN_EINVAL
    odd = BoxDecoder("Car", DEV, anchors=ot.generate_anchors("Car")[:3, :3, :1])
    assert odd.n_anchors == 9
    po, do = torch.rand(1, 1, 3, 3, device=DEV), torch.zeros(1, 7, 3, 3, device=DEV)
    assert int(odd.decode_device(po, do, 0.0, pre_nms_top_k=9)[2][0]) >= 1          # the flat layout takes it
    with pytest.raises(_lib.VoxelnetHipError, match="invalid argument"):
        odd.decode_device(po, do, 0.0, pre_nms_top_k=9, layout="site")
    with pytest.raises(_lib.VoxelnetHipError, match="invalid argument"):
        odd.candidates_device(po, do, 0.0, 9, layout="site")


# ----------------------------------------------------------------------------------------------- 3. the round trip
def _perfect_maps(pos, targets):
    """pos (B,h,w,2), targets (B,h,w,14) -> prob (B,2,h,w) = 0.05 + pos * (0.9 + distinct multiples of 2^-22), delta (B,14,h,w)
    = targets: the maps of a network that has fitted the loss's targets exactly, in the layout the loss reads"""
    p = pos.reshape(-1)
    rank = torch.cumsum(p, 0) * p                                            # 1, 2, ... over the positives
    assert float(rank.max()) < 2 ** 17                                       # 0.95 + rank * 2^-22 stays below 1 and exact in float32
    prob = (0.05 + p * (0.9 + rank * 2.0 ** -22)).reshape(pos.shape).permute(0, 3, 1, 2).contiguous()
    return prob, targets.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("grid", ["slice", "full"])
def test_round_trip_assign_decode_score(grid, kind):
    from voxelnet_amd.evaluate import DetectionEvaluator
    from voxelnet_amd.iou_loss import rpn_iou_loss
    from voxelnet_amd.predict import TRAINED_DECODE, BoxDecoder
    from voxelnet_amd.targets import TargetGenerator
    full = ot.generate_anchors("Car")
    anchors = full if grid == "full" else np.ascontiguousarray(full[100:124, 60:92])
    labels = C.round_trip_frames(anchors)
    n_gt = [len(f) for f in labels]
    assert n_gt == [2, 1, 0]
    gen = TargetGenerator("Car", DEV, anchors=anchors, assign=kind)
    pos, neg, targets = gen(labels)
    per_frame = pos.reshape(3, -1).sum(dim=1).tolist()
    print(f"{grid} {kind}: positives per frame {per_frame}")
    assert per_frame[0] >= 2 and per_frame[1] >= 1 and per_frame[2] == 0
    prob, delta = _perfect_maps(pos, targets)
    dec = BoxDecoder("Car", DEV, anchors=anchors)
    kw = dict(TRAINED_DECODE, score_thres=0.5, top_k=20)
    boxes, scores, counts = dec.decode_device(prob, delta, **kw)
    ev = DetectionEvaluator("Car", DEV, top_k=20)
    ev.update(boxes, scores, counts, labels)
    res = ev.compute()
    print(f"{grid} {kind}: counts {counts.tolist()}, BEV {res['bev']}, 3D {res['3d']}")
    assert counts.tolist() == n_gt                                      # one detection per ground truth, none elsewhere
    assert res["n_gt"]["all"] == 3 and res["n_det"] == 3
    for metric in ("bev", "3d"):
        for diff, ap in res[metric].items():
            assert ap == 1.0, (metric, diff, ap)
    # the flat reading of the same maps scrambles them: what the layout argument is for
    fb, fs, fc = dec.decode_device(prob, delta, **dict(kw, layout="flat"))
    ev2 = DetectionEvaluator("Car", DEV, top_k=20)
    ev2.update(fb, fs, fc, labels)
    assert ev2.compute()["3d"]["all"] < 0.5
    # the third consumer of the layout: the rotated-IoU loss decodes the same maps on the positives to the same boxes
    _, mean_iou = rpn_iou_loss(delta, pos, targets, gen._anchors_dev, "iou", "3d")
    print(f"{grid} {kind}: vn_rpn_iou_loss mean IoU {float(mean_iou):.7f}")
    assert float(mean_iou) >= 0.9999


# ------------------------------------------------------------------------------------ 4. RPN3D.evaluate / predict
def test_rpn3d_evaluate_with_trained_decode_reaches_the_layout_entry_point(monkeypatch):
    """the pattern of tests/test_gpu_detect.py::test_rpn3d_evaluate_passes_the_decode_arguments_on: evaluate(decode=
    TRAINED_DECODE) hands layout="site" to decode_device, which calls vn_rpn_detect_layout; RPN3D.predict(decode=) too"""
    from oracle import torch_ref as tr
    from voxelnet_amd import _lib
    from voxelnet_amd import model as M
    from voxelnet_amd import synth
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.evaluate import DetectionEvaluator
    from voxelnet_amd.predict import TRAINED_DECODE, BoxDecoder
    from voxelnet_amd.targets import generate_anchors
    from voxelnet_amd.voxelize import voxelize_device

    class Decoder(BoxDecoder):
        calls = []

        def decode_device(self, probs, deltas, **kw):
            out = BoxDecoder.decode_device(self, probs, deltas, **kw)
            flat = BoxDecoder.decode_device(self, _channels_last(probs.float()), _channels_last(deltas.float()),
                                            **dict(kw, layout="flat"))
            self.calls.append((kw, out, flat))
            return out
    names = []
    real = _lib.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    tg = grid_config("Car", H=16, W=24, oy=1.6)
    feats, coords = [], []
    for b in range(2):
        cloud = synth.synth_cloud("Car", k0=150 + 40 * b, seed=500 + b, grid=tg, overflow_frac=0.03)
        fb, cb, _ = voxelize_device(torch.from_numpy(cloud).to(DEV), tg, b, coord_cols=4)
        feats.append(fb)
        coords.append(cb)
    labels = [synth.synth_labels("Car", 3, 40 + b) for b in range(2)]
    batches = [(["000000", "000001"], labels, feats, None, coords, None, None)]
    before = M.get_precision()
    M.set_precision("bf16")
    try:
        m = M.RPN3D("Car")
        m.load_state_dict(tr.make_state_dict("Car"))
        m.feature_net._grid = replace(m.feature_net._grid, H=16, W=24)
        m = m.to(DEV).eval()
        dec = Decoder("Car", DEV, anchors=generate_anchors("Car")[:8, :12])
        ev = DetectionEvaluator("Car", DEV)
        monkeypatch.setattr(_lib, "call", recording)
        assert m.evaluate(batches, DEV, evaluator=ev, decoder=dec, decode=TRAINED_DECODE) is ev
        monkeypatch.setattr(_lib, "call", real)
        assert "vn_rpn_detect_layout" in names
        assert len(Decoder.calls) == 1
        kw, out, flat = Decoder.calls[0]
        assert kw == dict(top_k=ev.top_k, **TRAINED_DECODE) and kw["layout"] == "site"
        assert int(out[2].sum()) > 0
        for x, y in zip(out, flat):
            assert torch.equal(_bits(x), _bits(y))
        assert set(ev.compute()) == {"bev", "3d", "n_gt", "n_det"}
        # RPN3D.predict(decode=): the same detections as rows of strings
        m.__dict__["_decoder"] = BoxDecoder("Car", torch.device(DEV), anchors=generate_anchors("Car")[:8, :12])
        with torch.no_grad():
            prob, delta = m.detect(feats, coords)
        decode = dict(TRAINED_DECODE, top_k=ev.top_k)
        tag, rows = m.predict((["000000", "000001"],), prob, delta, decode=decode)
        wb, wsc = m.__dict__["_decoder"](prob, delta, **decode)
        assert tag == ["000000", "000001"] and [len(r) for r in rows] == [len(x) for x in wsc] and sum(len(x) for x in wsc) > 0
        for r, b_, s_ in zip(rows, wb, wsc):
            assert r.shape[1] == 9 and (r[:, 0] == "Car").all()
            assert np.allclose(r[:, 1:8].astype(np.float32), b_, rtol=1e-6) and np.allclose(r[:, 8].astype(np.float32), s_, rtol=1e-6)
        assert len(m.predict((["000000", "000001"],), prob, delta)[1]) == 2          # the default: the reference's tail
    finally:
        M.set_precision(before)
