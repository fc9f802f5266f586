"""GPU: the evaluation tail (csrc/detect.hip through vn_rpn_select_decode / vn_box_nms / vn_rpn_detect and
voxelnet_amd.predict) against the restatement tests/detect_ref.py.

Bars.  Selection: counts, scores and flat indices bit-exact and in order; decoded boxes within the bar
tests/test_gpu_predict.py uses (rtol 2.4e-7, atol 1e-6: the device's float32 exp may differ from NumPy's in the last
bit).  NMS: the reference walks THE DEVICE'S OWN float32 candidate boxes, read back, so a last-bit decode difference cannot
flip a decision; the test first asserts ON THE REFERENCE ALONE that no IoU it evaluated lies within 1e-7 of the threshold
(two orders above the 1e-9 device / reference agreement of the pair function), then keep_idx and
keep_counts must be equal exactly.  No seed had to be replaced: seeds 5 and 6 hold the guard in every combination
(smallest gap measured with NumPy-decoded boxes on the CPU: 2.1e-6).  Composition, determinism and parity with
vn_rpn_predict: bit-equal.

Stand-up mode and NaN fields: csrc/predict.hip's fminf / fmaxf drop a NaN corner (the rectangle comes out empty, IoU 0),
NumPy's min / max keep it (IoU NaN).  vn_box_nms restates the kernel verbatim, so the hand-made stand-up frames use
infinite and zero-width rows (on which both agree: a NaN IoU suppresses), and rows with a NaN field in rotated mode.

Scene "ped": the full Pedestrian anchor grid (N = 24,000 = 93 * 256 + 192) with tests/label_cases.py's clustered maps and
BoxDecoder("Pedestrian"): anchors of 0.6 x 0.8 and the class's anchor height 1.73 in the decoded z (a decoder with Car's 1.56
fails the selection test: the two differ by far more than the decode bar, asserted there).  The reference for that class is
the Car-pinned restatement with the class's constants."""
import functools

import numpy as np
import pytest
import torch

import detect_ref as D
import label_cases as L
from oracle import targets as ot

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 1e-7
MODES = {"standup": D.STANDUP, "rotated": D.ROTATED}
# scene -> (slice of the class's generate_anchors, score_thres, pre_top_k)
SCENES = {"dense": ((slice(0, 24), slice(0, 20)), 0.25, 512),
          "spread": ((slice(None, None, 4), slice(None, None, 4)), 0.70, 1024),
          "wide": ((slice(None, None, 2), slice(None, None, 2)), 0.70, 4096),
          "ped": ((slice(None), slice(None)), 0.50, 512)}
SCENE_CLASS = {"ped": "Pedestrian"}          # every other scene: "Car"
SEEDS = (5, 6)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _anchors(scene):
    sl = SCENES[scene][0]
    return np.ascontiguousarray(ot.generate_anchors(SCENE_CLASS.get(scene, "Car"))[sl[0], sl[1]])


@functools.lru_cache(maxsize=None)
def _decoder(scene):
    from voxelnet_amd.predict import BoxDecoder
    return BoxDecoder(SCENE_CLASS.get(scene, "Car"), DEV, anchors=None if scene in ("full", "ped") else _anchors(scene))


@functools.lru_cache(maxsize=None)
def _maps(scene, seed):
    """tests/test_gpu_predict.py's random maps on the scene's anchors: B = 2"""
    h, w = (200, 176) if scene == "full" else _anchors(scene).shape[:2]
    if scene == "ped":          # clustered candidates: 96 neighbouring anchors at 0.96.., the rest below 0.9
        return L.clustered_maps((h, w), seed)
    rng = np.random.default_rng(seed)
    probs = rng.random((2, 2, h, w)).astype(np.float32)
    deltas = (rng.standard_normal((2, 14, h, w)) * 0.3).astype(np.float32)
    return probs, deltas


@functools.lru_cache(maxsize=None)
def _candidates(scene, seed):
    """the device's candidates of the scene, read back once: (boxes, scores, idx, counts) NumPy"""
    probs, deltas = _maps(scene, seed)
    _, thres, pre = SCENES[scene]
    out = _decoder(scene).candidates_device(_dev(probs), _dev(deltas), thres, pre)
    return tuple(t.cpu().numpy() for t in out)


def _check_selection(probs, deltas, anchors, thres, pre, got, cls_name="Car"):
    boxes, scores, idx, counts = got
    B = probs.shape[0]
    assert boxes.shape == (B, pre, 7) and scores.shape == (B, pre) and idx.shape == (B, pre) and counts.shape == (B,)
    for b in range(B):
        want = D.select(probs[b], thres, pre)
        n = len(want)
        assert counts[b] == n, (b, counts[b], n)
        assert np.array_equal(idx[b, :n], want), b
        assert np.array_equal(_u32(scores[b, :n]), _u32(probs[b].reshape(-1)[want])), b
        np.testing.assert_allclose(boxes[b, :n], D.decode(deltas[b], anchors, want, cls_name), rtol=2.4e-7, atol=1e-6)
        assert (boxes[b, n:] == 0).all() and (scores[b, n:] == 0).all() and (idx[b, n:] == 0).all()          # untouched rows
    return counts


# ------------------------------------------------------------------------------------------------ 1. selection
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_selection_matches_reference(scene, seed):
    probs, deltas = _maps(scene, seed)
    _, thres, pre = SCENES[scene]
    cls = SCENE_CLASS.get(scene, "Car")
    counts = _check_selection(probs, deltas, _anchors(scene), thres, pre, _candidates(scene, seed), cls)
    n_cand = (probs.reshape(2, -1) >= np.float32(thres)).sum(axis=1)
    assert (counts == pre).all() and (n_cand > pre).all()          # the cut really truncates
    if cls != "Car":
        # the class's anchor height is in the decoded z: with Car's 1.56 the same rows lie far outside the decode bar
        assert _decoder(scene).anchor_h == ot.CLASSES[cls]["h"] == 1.73 and _anchors(scene).shape == (100, 120, 2, 7)
        for b in range(2):
            want = D.select(probs[b], thres, pre)
            z, z_car = (D.decode(deltas[b], _anchors(scene), want, c)[:, 2].astype(np.float64) for c in (cls, "Car"))
            assert (np.abs(z - z_car) > 100 * (1e-6 + 2.4e-7 * np.abs(z))).mean() > 0.9


def test_selection_pool_larger_than_the_candidates_and_empty():
    probs, deltas = _maps("dense", 5)
    dec = _decoder("dense")
    got = tuple(t.cpu().numpy() for t in dec.candidates_device(_dev(probs), _dev(deltas), 0.25, 1024))
    counts = _check_selection(probs, deltas, _anchors("dense"), 0.25, 1024, got)
    assert (counts == (probs.reshape(2, -1) >= np.float32(0.25)).sum(axis=1)).all() and (counts < 1024).all()
    got = tuple(t.cpu().numpy() for t in dec.candidates_device(_dev(probs), _dev(deltas), 2.0, 64))
    assert (_check_selection(probs, deltas, _anchors("dense"), 2.0, 64, got) == 0).all()
    # pre_top_k = 1: the arg-max
    got = tuple(t.cpu().numpy() for t in dec.candidates_device(_dev(probs), _dev(deltas), 0.25, 1))
    assert (_check_selection(probs, deltas, _anchors("dense"), 0.25, 1, got) == 1).all()


def test_selection_ties_at_the_top_and_across_the_cut():
    """equal scores: the larger flat index first — at the top, and inside a tie group that straddles the cut (the radix
    selection has to descend into the index word); -0.0 / +0.0 / NaN scores"""
    probs, deltas = _maps("dense", 6)
    probs = probs.copy()
    pre, thres = 512, 0.25
    flat = probs.reshape(2, -1)
    rng = np.random.default_rng(17)
    for b in range(2):
        s = np.sort(flat[b])[::-1]
        v = s[500]                                             # 500 scores above v: a group of 40 at v covers ranks 501..541
        low = np.where(flat[b] < v)[0]
        flat[b, rng.choice(low, 40, replace=False)] = v
        top = rng.choice(np.where(flat[b] < v)[0], 5, replace=False)
        flat[b, top] = 1.0
        order = D.select(flat[b], -np.inf, flat.shape[1])
        sv = flat[b][order]
        assert sv[0] == sv[4] == 1.0 and sv[pre - 1] == sv[pre] == v          # the cut falls inside the group
    flat[1, 3] = np.nan
    got = tuple(t.cpu().numpy() for t in _decoder("dense").candidates_device(_dev(probs), _dev(deltas), thres, pre))
    _check_selection(probs, deltas, _anchors("dense"), thres, pre, got)
    # a map of zeros of both signs and a NaN, everything a candidate at threshold 0: pure index order
    z = np.zeros_like(probs)
    z.reshape(2, -1)[:, ::3] = -0.0
    z.reshape(2, -1)[0, 100] = np.nan
    got = tuple(t.cpu().numpy() for t in _decoder("dense").candidates_device(_dev(z), _dev(deltas), 0.0, 700))
    _check_selection(z, deltas, _anchors("dense"), 0.0, 700, got)
    assert got[2][1, :3].tolist() == [959, 958, 957] and np.signbit(got[1][1, :6]).tolist() == [False, False, True] * 2


def test_selection_full_size():
    """all 70,400 anchors are candidates (score_thres 0), pre_top_k 4096"""
    probs, deltas = _maps("full", 5)
    got = tuple(t.cpu().numpy() for t in _decoder("full").candidates_device(_dev(probs), _dev(deltas), 0.0, 4096))
    counts = _check_selection(probs, deltas, ot.generate_anchors("Car"), 0.0, 4096, got)
    assert (counts == 4096).all()


# ------------------------------------------------------------------------------------------------ 2. vn_box_nms
def _nms_device(boxes, counts, mode, thr, post):
    from voxelnet_amd.predict import nms_device
    keep, kc = nms_device(_dev(boxes), _dev(np.asarray(counts, dtype=np.int32)), mode, thr, post)
    assert keep.dtype == torch.int32 and kc.dtype == torch.int32 and tuple(keep.shape) == (boxes.shape[0], post)
    return keep.cpu().numpy(), kc.cpu().numpy()


def _check_nms(boxes, counts, mode, thr, post, caches=None):
    keep, kc = _nms_device(boxes, counts, mode, thr, post)
    kept = []
    for b in range(boxes.shape[0]):
        n = min(max(int(counts[b]), 0), boxes.shape[1])
        want, gap = D.nms(boxes[b, :n], MODES[mode], thr, post, None if caches is None else caches[b])
        print(f"{mode} thr {thr} post {post} sample {b}: kept {len(want)}, smallest |IoU - thr| {gap:.3e}")
        assert gap > MARGIN, (b, gap)          # on the reference alone: no decision within the margin
        assert kc[b] == len(want), (b, kc[b], len(want))
        assert keep[b, :len(want)].tolist() == want, b
        assert (keep[b, len(want):] == -1).all(), b
        kept.append(len(want))
    return kept


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_box_nms_matches_reference(scene, seed, mode):
    boxes, _, _, counts = _candidates(scene, seed)
    caches = [{}, {}]          # the rotated IoUs of a sample, shared by the four (threshold, cap) combinations
    for thr in (0.1, 0.5):
        for post in (64, 20):
            kept = _check_nms(boxes, counts, mode, thr, post, caches)
            if scene == "ped":                       # the clustered candidates lead the pool: the walk suppresses among them
                lead = [len(D.nms(boxes[b, :96], MODES[mode], thr, 96, caches[b])[0]) for b in range(2)]
                assert all(k < 96 for k in lead) and all(k >= 1 for k in kept)
            elif scene != "dense":
                assert kept == [post, post]          # spread and wide hit the cap
            elif thr == 0.1 and post == 64:
                assert all(k < 64 for k in kept)     # dense at 0.1: the whole pool is walked


def _hand_frames(mode):
    car = [20.0, 3.0, -1.6, 1.5, 1.6, 3.9, 0.3]

    def moved(dx=0.0, dy=0.0, **kw):
        q = list(car)
        q[0] += dx
        q[1] += dy
        for k, v in kw.items():
            q[int(k[1:])] = v
        return q
    K = 128
    frames, counts = [], []

    def add(rows, count=None):
        a = np.zeros((K, 7), dtype=np.float32)
        rows = np.array(rows, dtype=np.float32).reshape(-1, 7)
        a[:len(rows)] = rows
        frames.append(a)
        counts.append(len(rows) if count is None else count)
    add([car], 0)                                                              # count 0: the row is not looked at
    add([car])                                                                 # count 1
    add([moved(dx=6.0 * (k % 16), dy=5.0 * (k // 16)) for k in range(K)], K + 7)   # count > K is K
    add([car] * 100)                                                           # 100 identical boxes
    add([car, moved(dx=1.95 * np.cos(0.3), dy=1.95 * np.sin(0.3)), moved(dx=4.6 * np.cos(0.3), dy=4.6 * np.sin(0.3))])   # chain
    add([moved(dx=7.0 * k) for k in range(5)], -3)                             # a negative count is 0
    if mode == "rotated":          # invalid rows are never kept and suppress nothing
        add([moved(f0=np.nan), moved(f4=0.0), car, moved(dx=0.2), moved(f6=np.inf), moved(dx=9.0, f3=-1.0), moved(dx=9.0),
             moved(dx=9.1, f5=np.nan)])
    else:                          # a zero-width row is a rectangle like any other; an infinite coordinate: IoU NaN, which suppresses
        add([moved(f4=0.0), car, moved(dx=0.2), moved(dx=9.0, f0=np.inf), moved(dx=9.0)])
        add([moved(f0=np.inf), car, moved(dx=30.0)])
    return np.stack(frames), np.array(counts, dtype=np.int32)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_box_nms_hand_made_frames(mode):
    boxes, counts = _hand_frames(mode)
    kept = _check_nms(boxes, counts, mode, 0.1, 64)
    assert kept[:6] == [0, 1, 64, 1, 2, 0]
    assert kept[6:] == ([2] if mode == "rotated" else [2, 1])
    assert _check_nms(boxes, counts, mode, 0.1, 3)[:6] == [0, 1, 3, 1, 2, 0]
    # a negative threshold: IoU 0 <= thr is false, every later row goes (no far-pair shortcut)
    assert _check_nms(boxes[2:3], counts[2:3], mode, -0.5, 64) == [1]


def test_box_nms_side_by_side_at_45_degrees():
    r = np.pi / 4
    a = [20.0, 3.0, -1.6, 1.5, 1.6, 3.9, r]
    b = [20.0 - 2.4 * np.sin(r), 3.0 + 2.4 * np.cos(r), -1.6, 1.5, 1.6, 3.9, r]
    boxes = np.array([[a, b]], dtype=np.float32)
    assert _check_nms(boxes, [2], "rotated", 0.1, 20) == [2]
    assert _check_nms(boxes, [2], "standup", 0.1, 20) == [1]


# ------------------------------------------------------------------------- 3. vn_rpn_detect = the composition
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_detect_is_the_composition_and_deterministic(scene, mode):
    from voxelnet_amd.predict import nms_device
    probs, deltas = _maps(scene, 5)
    _, thres, pre = SCENES[scene]
    dec = _decoder(scene)
    p, d = _dev(probs), _dev(deltas)
    cb, cs, _, cc = dec.candidates_device(p, d, thres, pre)
    for thr, post in ((0.1, 64), (0.5, 20)):
        keep, kc = nms_device(cb, cc, mode, thr, post)
        boxes, scores, counts = dec.decode_device(p, d, thres, thr, post, nms=mode, pre_nms_top_k=pre)
        assert tuple(boxes.shape) == (2, post, 7) and tuple(scores.shape) == (2, post)
        assert torch.equal(counts, kc) and int(kc.min()) > 0
        for b in range(2):
            n = int(kc[b])
            rows = keep[b, :n].long()
            assert torch.equal(boxes[b, :n].view(torch.int32), cb[b][rows].view(torch.int32)), b
            assert torch.equal(scores[b, :n].view(torch.int32), cs[b][rows].view(torch.int32)), b
            assert (boxes[b, n:] == 0).all() and (scores[b, n:] == 0).all()
            assert (scores[b, :n - 1] >= scores[b, 1:n]).all()
        for _ in range(2):          # three calls in all: bit-equal
            again = dec.decode_device(p, d, thres, thr, post, nms=mode, pre_nms_top_k=pre)
            for x, y in zip((boxes, scores, counts), again):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_detect_matches_reference_end_to_end():
    """the whole chain against detect_ref.detect on the spread scene (its own NumPy decoding): same detections"""
    probs, deltas = _maps("spread", 5)
    _, thres, pre = SCENES["spread"]
    for mode in sorted(MODES):
        boxes, scores = _decoder("spread")(_dev(probs), _dev(deltas), thres, 0.1, 20, nms=mode, pre_nms_top_k=pre)
        for b in range(2):
            rb, rs = D.detect(probs[b], deltas[b], _anchors("spread"), thres, pre, MODES[mode], 0.1, 20)
            assert np.array_equal(_u32(scores[b]), _u32(rs)), (mode, b)
            np.testing.assert_allclose(boxes[b], rb, rtol=2.4e-7, atol=1e-6)


# ------------------------------------------------------- 4. stand-up, pre = post = 20: bit-identical to vn_rpn_predict
@pytest.mark.parametrize("which", ["fixture maps", "dense random with ties"])
def test_standup_pre_equals_post_is_vn_rpn_predict(which):
    if which == "fixture maps":
        from test_oracle_predict import maps
        probs, deltas = maps()
    else:          # tests/test_gpu_predict.py::test_predict_matches_oracle_random, dense
        rng = np.random.default_rng(6)
        probs = rng.random((2, 2, 200, 176)).astype(np.float32)
        deltas = (rng.standard_normal((2, 14, 200, 176)) * 0.3).astype(np.float32)
        probs[0, 0, 3, 5:9] = 1.0
        probs[1, 1, 7, 7] = 1.0
    dec = _decoder("full")
    p, d = _dev(probs), _dev(deltas)
    old = dec.decode_device(p, d)
    new = dec.decode_device(p, d, pre_nms_top_k=20)
    assert int(old[2].sum()) > 0
    for x, y in zip(old, new):
        assert torch.equal(x, y) and torch.equal(x.view(torch.int32), y.view(torch.int32))
    old = dec.decode_device(p, d, 0.9, 0.3, 64)
    new = dec.decode_device(p, d, 0.9, 0.3, 64, pre_nms_top_k=64)
    for x, y in zip(old, new):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ------------------------------------------------------------------------------------ 5. the three-car cluster
def _cluster_maps():
    """three well-separated cars, each fired on by 30 neighbouring anchors whose deltas put the box on the car (a few
    centimetres of jitter), at scores 0.99.., 0.98.., 0.97..; everything else at 0.5"""
    anchors = ot.generate_anchors("Car").reshape(-1, 7)
    rng = np.random.default_rng(1)
    probs = np.full((1, 2, 200, 176), 0.5, dtype=np.float32)
    deltas = np.zeros((1, 14, 200, 176), dtype=np.float32)
    pf, df = probs.reshape(1, -1), deltas.reshape(1, -1, 7)
    diag = np.sqrt(1.6 ** 2 + 3.9 ** 2)
    for c, (x, y) in enumerate([(15.0, -20.0), (35.0, 4.0), (55.0, 25.0)]):
        near = np.argsort(np.hypot(anchors[:, 0] - x, anchors[:, 1] - y) + 100.0 * (anchors[:, 6] != 0), kind="stable")[:30]
        for k, j in enumerate(near):
            df[0, j, 0] = (x + rng.uniform(-0.05, 0.05) - anchors[j, 0]) / diag
            df[0, j, 1] = (y + rng.uniform(-0.05, 0.05) - anchors[j, 1]) / diag
            pf[0, j] = 0.99 - 0.01 * c + 1e-4 * k
    return probs, deltas


def test_three_clustered_cars_need_a_wider_pool():
    probs, deltas = _cluster_maps()
    dec = _decoder("full")
    p, d = _dev(probs), _dev(deltas)
    boxes, scores = dec(p, d)
    assert len(scores[0]) == 1 and abs(boxes[0][0, 0] - 15.0) < 0.1          # the reference's tail: 20 candidates, one car
    for mode in sorted(MODES):
        boxes, scores = dec(p, d, nms=mode, pre_nms_top_k=90)
        assert len(scores[0]) == 3, mode
        assert np.allclose(boxes[0][:, 0], [15.0, 35.0, 55.0], atol=0.1) and np.allclose(boxes[0][:, 1], [-20.0, 4.0, 25.0], atol=0.1)
        rb, rs = D.detect(probs[0], deltas[0], ot.generate_anchors("Car"), 0.96, 90, MODES[mode], 0.1, 20)
        assert np.array_equal(_u32(scores[0]), _u32(rs))


# ---------------------------------------------------------------------------------------- 6. the Python surface
def test_default_arguments_are_the_unchanged_vn_rpn_predict_call():
    from test_oracle_predict import maps
    from voxelnet_amd import _lib
    probs, deltas = maps()
    dec = _decoder("full")
    p, d = _dev(probs), _dev(deltas)
    B, N = 3, dec.n_anchors
    boxes = torch.zeros((B, 20, 7), dtype=torch.float32, device=DEV)
    scores = torch.zeros((B, 20), dtype=torch.float32, device=DEV)
    counts = torch.zeros(B, dtype=torch.int32, device=DEV)
    nbytes = _lib.load().vn_rpn_predict_workspace_bytes(B, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.call("vn_rpn_predict", p.data_ptr(), d.data_ptr(), dec._anchors_dev.data_ptr(), B, N, 0.96, 0.1, 20, dec.anchor_h,
              boxes.data_ptr(), scores.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, _lib.raw_stream())
    for got in (dec.decode_device(p, d), dec.decode_device(p, d, nms="standup", pre_nms_top_k=None)):
        for x, y in zip((boxes, scores, counts), got):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    ch = counts.cpu().numpy()
    assert ch.sum() > 0 and ch[2] == 0
    for b in range(B):
        assert (boxes[b, ch[b]:] == 0).all() and (scores[b, ch[b]:] == 0).all()
    lb, ls = dec(p, d, nms="rotated", pre_nms_top_k=256)
    assert [len(s) for s in ls] == dec.decode_device(p, d, nms="rotated", pre_nms_top_k=256)[2].tolist()


def test_surface_argument_errors():
    from voxelnet_amd import _lib
    from voxelnet_amd.predict import nms_device
    probs, deltas = _maps("dense", 5)
    dec = _decoder("dense")
    p, d = _dev(probs), _dev(deltas)
    with pytest.raises(_lib.VoxelnetHipError):
        dec.decode_device(p.cpu(), d, nms="rotated")
    with pytest.raises(_lib.VoxelnetHipError):
        dec.candidates_device(p, d.cpu(), 0.5, 64)
    with pytest.raises(_lib.VoxelnetHipError):
        nms_device(torch.zeros(1, 4, 7), torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        dec.decode_device(p, d, nms="3d")
    with pytest.raises(ValueError):
        dec.decode_device(p, d, nms="rotated", pre_nms_top_k=4097)
    with pytest.raises(ValueError):
        dec.decode_device(p, d, nms="rotated", top_k=65)
    with pytest.raises(ValueError):
        dec.decode_device(p, d, nms="rotated", nms_thres=float("nan"))
    with pytest.raises(ValueError):
        dec.candidates_device(p, d, 0.5, 0)
    with pytest.raises(ValueError):
        nms_device(torch.zeros(1, 4097, 7, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        nms_device(torch.zeros(1, 4, 7, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), "rotated", 0.1, 65)


class _Recorder:
    """an evaluator that keeps what it is handed and passes it on"""

    def __init__(self, inner):
        self.inner, self.top_k, self.seen = inner, inner.top_k, []

    def update(self, boxes, scores, counts, labels):
        self.seen.append((boxes, scores, counts))
        return self.inner.update(boxes, scores, counts, labels)


def test_rpn3d_evaluate_passes_the_decode_arguments_on():
    from dataclasses import replace

    from oracle import torch_ref as tr
    from voxelnet_amd import model as M
    from voxelnet_amd import synth
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.evaluate import DetectionEvaluator
    from voxelnet_amd.predict import EVAL_DECODE, BoxDecoder
    from voxelnet_amd.targets import generate_anchors
    from voxelnet_amd.voxelize import voxelize_device

    class Decoder(BoxDecoder):          # keeps every call's keyword arguments, and a second decoding of the same maps
        calls = []

        def decode_device(self, probs, deltas, **kw):
            out = BoxDecoder.decode_device(self, probs, deltas, **kw)
            self.calls.append((kw, out, BoxDecoder.decode_device(self, probs, deltas, **kw)))
            return out
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
        for decode in (EVAL_DECODE, None):
            del Decoder.calls[:]
            rec = _Recorder(DetectionEvaluator("Car", DEV))
            assert m.evaluate(batches, DEV, evaluator=rec, decoder=dec, decode=decode) is rec and not m.training
            assert len(rec.seen) == 1 and len(Decoder.calls) == 1
            kw, out, again = Decoder.calls[0]
            assert kw == dict(top_k=rec.top_k, **(decode or {}))
            for seen, x, y in zip(rec.seen[0], out, again):          # the evaluator got exactly what decode_device returns
                assert seen is x and torch.equal(x.view(torch.int32), y.view(torch.int32))
            assert tuple(out[0].shape) == (2, rec.top_k, 7)
            res = rec.inner.compute()
            assert set(res) == {"bev", "3d", "n_gt", "n_det"} and res["n_gt"]["all"] == 6
            if decode is not None:
                assert int(out[2].sum()) > 0          # at 0.1 even an untrained head has detections to score
        with pytest.raises(ValueError):
            m.evaluate(batches, DEV, decoder=dec, decode=dict(top_k=5))
    finally:
        M.set_precision(before)
