"""Device inference tail (csrc/predict.hip through vn_rpn_predict / voxelnet_amd.predict / RPN3D.predict) against the
oracle (oracle/predict.py, pinned to the reference by tests/golden/predict_car.npz) and the fixture itself.
Bar: the kept detections — same count, same scores (bit-exact), in the same order; boxes within 2 fp32 ulp of the
reference's (the device's float32 exp / float64 sin, cos may differ from NumPy's in the last bit).

Off the Car grid and with an NMS that has work to do (tests/label_cases.py: clustered candidates on the Pedestrian,
Cyclist and Car grids and on slices of 130 and 270 anchors; what the maps contain — the reference keeps fewer boxes than it
selects, no IoU of its walk within 1e-4 of the threshold — is asserted on the reference alone by
tests/test_label_cases_host.py and again here before the device is compared).  oracle/predict.py hard-codes the
reference's constants, so other top_k and thresholds are held against tests/detect_ref.py in stand-up mode with
pre_top_k = post_top_k = top_k.  The oracle for Pedestrian and Cyclist is the Car-pinned code with their constants; there is
no golden of their own.  Same bars."""
import os

import numpy as np
import pytest
import torch

import label_cases as L
from oracle import predict as op
from oracle import targets as ot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "predict_car.npz")


def _maps():
    from test_oracle_predict import maps
    return maps()


def test_predict_matches_reference_fixture():
    from voxelnet_amd.predict import BoxDecoder
    g = np.load(GOLD)
    probs, deltas = _maps()
    boxes, scores = BoxDecoder("Car", DEV)(torch.from_numpy(probs).to(DEV), torch.from_numpy(deltas).to(DEV))
    for b in range(int(g["n_samples"])):
        assert np.array_equal(scores[b], g[f"ret_scores{b}"]), b
        assert boxes[b].shape == g[f"ret_boxes{b}"].shape
        np.testing.assert_allclose(boxes[b], g[f"ret_boxes{b}"], rtol=2.4e-7, atol=1e-6)


@pytest.mark.parametrize("seed,dense", [(5, False), (6, True)])
def test_predict_matches_oracle_random(seed, dense):
    """dense: thousands of candidates above the threshold, exact score ties, degenerate boxes"""
    from voxelnet_amd.predict import BoxDecoder
    rng = np.random.default_rng(seed)
    B, h, w = 2, 200, 176
    probs = (rng.random((B, 2, h, w)) * (1.0 if dense else 0.97)).astype(np.float32)
    deltas = (rng.standard_normal((B, 14, h, w)) * 0.3).astype(np.float32)
    if dense:
        probs[0, 0, 3, 5:9] = 1.0                 # ties: the larger flat index first (oracle/predict.py)
        probs[1, 1, 7, 7] = 1.0
    anchors = ot.generate_anchors("Car")
    rb, rs = op.predict_boxes(probs, deltas, anchors)
    boxes, scores = BoxDecoder("Car", DEV)(torch.from_numpy(probs).to(DEV), torch.from_numpy(deltas).to(DEV))
    for b in range(B):
        assert np.array_equal(scores[b], rs[b]), b
        np.testing.assert_allclose(boxes[b], rb[b].reshape(-1, 7), rtol=2.4e-7, atol=1e-6)


def test_rpn3d_predict_returns_the_reference_format():
    from voxelnet_amd import model as M
    probs, deltas = _maps()
    model = M.RPN3D("Car").to(DEV)
    data = (["000001", "000002", "000003"], None, None, None, None, None, None)
    tag, ret = model.predict(data, torch.from_numpy(probs).to(DEV), torch.from_numpy(deltas).to(DEV))
    g = np.load(GOLD)
    assert tag == data[0] and len(ret) == 3
    for b in range(3):
        n = g[f"ret_boxes{b}"].shape[0]
        assert ret[b].shape == (n, 9) if n else ret[b].shape[0] == 0
        if n:
            assert ret[b].dtype.kind == "U" and (ret[b][:, 0] == "Car").all()
            np.testing.assert_allclose(ret[b][:, 8].astype(np.float32), g[f"ret_scores{b}"], rtol=1e-6)
    with pytest.raises(NotImplementedError):
        model.predict(data, torch.from_numpy(probs).to(DEV), torch.from_numpy(deltas).to(DEV), summary=True)
    with pytest.raises(M._lib.VoxelnetHipError):
        model.predict(data, torch.from_numpy(probs), torch.from_numpy(deltas))


# ------------------------------------------------------------------------------------- off the Car anchor grid
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _decoder(case):
    from voxelnet_amd.predict import BoxDecoder
    dec = BoxDecoder(case.cls_name, DEV, anchors=None if case.grid == "full" else case.anchors)
    assert np.array_equal(dec.anchors, case.anchors) and dec.anchor_h == ot.CLASSES[case.cls_name]["h"]
    return dec


def _check_against_walk(dec, case, probs, deltas, score_thres, nms_thres, top_k):
    """decode_device against detect_ref's stand-up walk with pre = post = top_k -> per sample (selected, kept)"""
    boxes, scores, counts = (t.cpu().numpy() for t in dec.decode_device(_dev(probs), _dev(deltas), score_thres, nms_thres, top_k))
    assert boxes.shape == (2, top_k, 7) and scores.shape == (2, top_k) and counts.shape == (2,)
    out = []
    for b in range(2):
        rb, rs, n_sel, gap = L.reference_walk(probs[b], deltas[b], case.anchors, case.cls_name, score_thres, nms_thres, top_k)
        print(f"{case.id} sample {b} thres {score_thres} nms {nms_thres} top_k {top_k}: selected {n_sel}, kept {len(rs)}, "
              f"smallest |IoU - thr| {gap:.2e}")
        assert gap > L.NMS_MARGIN, (b, gap)          # on the reference alone
        n = len(rs)
        assert counts[b] == n, (b, counts[b], n)
        assert np.array_equal(scores[b, :n].view(np.uint32), rs.view(np.uint32)), b
        np.testing.assert_allclose(boxes[b, :n], rb, rtol=2.4e-7, atol=1e-6)
        assert (boxes[b, n:] == 0).all() and (scores[b, n:] == 0).all()
        out.append((n_sel, n))
    return out


_DEC = L.decode_cases()


@pytest.mark.parametrize("case", _DEC, ids=[c.id for c in _DEC])
def test_predict_matches_oracle_on_clustered_maps(case):
    """the reference's constants: oracle.predict.predict_boxes with the class's anchors and anchor height"""
    rb, rs = case.ref
    boxes, scores = _decoder(case)(_dev(case.probs), _dev(case.deltas))
    n_cand = case.candidates()
    for b in range(2):
        assert np.array_equal(scores[b], rs[b]), b
        assert boxes[b].shape == rb[b].shape
        np.testing.assert_allclose(boxes[b], rb[b], rtol=2.4e-7, atol=1e-6)
        assert 1 <= len(scores[b]) < min(n_cand[b], op.NMS_POST_TOPK)          # the suppression was real
        assert (np.diff(scores[b]) <= 0).all()


@pytest.mark.parametrize("cls,grid", [("Pedestrian", "full"), ("Cyclist", (9, 15)), ("Pedestrian", (5, 13)), ("Car", "full")])
def test_predict_top_k_and_thresholds(cls, grid):
    """top_k 1, 20 and VN_PREDICT_MAX_TOPK = 64, score and NMS thresholds other than the reference's"""
    case = L.decode_case(cls, grid, L.DECODE_SEEDS[0])
    dec = _decoder(case)
    if cls == "Car":          # with the reference's constants detect_ref's walk IS oracle.predict
        for b in range(2):
            rb, rs, _, _ = L.reference_walk(case.probs[b], case.deltas[b], case.anchors, cls, op.SCORE_THRES, op.NMS_THRES, 20)
            assert np.array_equal(rs, case.ref[1][b]) and np.array_equal(rb, case.ref[0][b])
    for score_thres, nms_thres, top_k in L.DECODE_PARAMS:
        got = _check_against_walk(dec, case, case.probs, case.deltas, score_thres, nms_thres, top_k)
        n_cand = case.candidates(score_thres)
        for b, (n_sel, n) in enumerate(got):
            assert n_sel == min(top_k, n_cand[b])
            if top_k > 1 and (score_thres, nms_thres) == (op.SCORE_THRES, op.NMS_THRES):
                assert n < n_sel


@pytest.mark.parametrize("cls,grid", [("Pedestrian", "full"), ("Cyclist", (9, 15))])
def test_predict_few_and_no_candidates(cls, grid):
    case = L.decode_case(cls, grid, L.DECODE_SEEDS[1])
    dec = _decoder(case)
    flat = case.probs.reshape(2, -1)
    thr = float(np.sort(flat[0])[-5])          # EQUAL to the fifth best score of sample 0: `>=` keeps it
    assert np.float32(thr) == np.sort(flat[0])[-5] and (flat[0] >= np.float32(thr)).sum() == 5
    # an NMS threshold no IoU passes: all five come back, the last one at the threshold itself
    for top_k in (20, 64):
        got = _check_against_walk(dec, case, case.probs, case.deltas, thr, 2.0, top_k)
        assert got[0] == (5, 5) and got[1][0] == int((flat[1] >= np.float32(thr)).sum()) < top_k
    scores = dec.decode_device(_dev(case.probs), _dev(case.deltas), thr, 2.0, 20)[1].cpu().numpy()
    assert scores[0, 4] == np.float32(thr) and scores[0, 5] == 0
    _check_against_walk(dec, case, case.probs, case.deltas, thr, op.NMS_THRES, 20)          # and with a real NMS
    # no candidate at all: counts 0, outputs still zero
    for top_k in (1, 20, 64):
        boxes, scores, counts = dec.decode_device(_dev(case.probs), _dev(case.deltas), 2.0, op.NMS_THRES, top_k)
        assert (counts == 0).all() and (boxes == 0).all() and (scores == 0).all()
    lb, ls = dec(_dev(case.probs), _dev(case.deltas), 2.0)
    assert [len(s) for s in ls] == [0, 0] and lb[0].shape == (0, 7)


@pytest.mark.parametrize("cls,grid", [("Pedestrian", "full"), ("Cyclist", "full"), ("Cyclist", (9, 15))])
def test_predict_exact_score_ties_inside_a_cluster(cls, grid):
    """four neighbouring flat indices at the top score, seven equal scores straddling the top_k cut: the larger flat index
    goes first (oracle/predict.py), at the top and at the cut"""
    case = L.decode_case(cls, grid, L.DECODE_SEEDS[0])
    probs, deltas = L.tied_maps(case, 20)
    for b in range(2):
        f = probs[b].reshape(-1)
        order = np.lexsort((np.arange(f.size), f))[::-1]
        assert f[order[17]] == f[order[23]] and f[order[16]] > f[order[17]] and f[order[23]] > f[order[24]]
        assert (f[order[:6]] == np.float32(0.9995)).sum() == 4
    dec = _decoder(case)
    _check_against_walk(dec, case, probs, deltas, op.SCORE_THRES, op.NMS_THRES, 20)
    rb, rs = op.predict_boxes(probs, deltas, case.anchors, cls)
    boxes, scores = dec(_dev(probs), _dev(deltas))
    for b in range(2):
        assert np.array_equal(scores[b], rs[b]), b
        np.testing.assert_allclose(boxes[b], rb[b].reshape(-1, 7), rtol=2.4e-7, atol=1e-6)
    # NMS off (no IoU passes 2): the 20 selected come back in selection order, the tie groups in descending flat index
    got = dec.decode_device(_dev(probs), _dev(deltas), op.SCORE_THRES, 2.0, 20)
    _check_against_walk(dec, case, probs, deltas, op.SCORE_THRES, 2.0, 20)
    assert (got[2] == 20).all()


def test_predict_routes_agree_on_the_pedestrian_grid():
    """vn_rpn_predict and vn_rpn_detect (stand-up, pre_nms_top_k = top_k): bit-identical boxes, scores and counts"""
    case = L.decode_case("Pedestrian", "full", L.DECODE_SEEDS[0])
    dec = _decoder(case)
    maps = [(case.probs, case.deltas), L.tied_maps(case, 20)]
    for probs, deltas in maps:
        p, d = _dev(probs), _dev(deltas)
        for score_thres, nms_thres, top_k in L.DECODE_PARAMS:
            old = dec.decode_device(p, d, score_thres, nms_thres, top_k)
            new = dec.decode_device(p, d, score_thres, nms_thres, top_k, nms="standup", pre_nms_top_k=top_k)
            assert int(old[2].sum()) > 0
            for x, y in zip(old, new):
                assert x.shape == y.shape and torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_rpn3d_pedestrian_predict_raises_about_the_anchor_count():
    """RPN3D("Pedestrian") emits 200 x 240 maps, its anchor grid has 100 x 120 cells (the reference's own mismatch): a
    ValueError, not boxes decoded against the wrong anchors"""
    from voxelnet_amd import model as M
    from voxelnet_amd.config import grid_config
    model = M.RPN3D("Pedestrian")
    g = grid_config("Pedestrian")
    h, w = g.H // g.block1_stride, g.W // g.block1_stride
    assert (h, w) == (200, 240) and tuple(model.rpn_output_shape) == (100, 120)
    probs = torch.zeros((1, 2, h, w), device=DEV)
    deltas = torch.zeros((1, 14, h, w), device=DEV)
    with pytest.raises(ValueError, match="anchors"):
        model.predict((["000001"],), probs, deltas)
