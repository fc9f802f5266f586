"""GPU: Soft-NMS (csrc/soft_nms.hip through vn_box_soft_nms, predict.SoftNMS / soft_nms_device, the soft_nms= keyword) against
the float64 restatement tests/soft_nms_ref.py.

Bars.  keep_idx and keep_counts equal; keep_scores within |dev - ref| <= ref * (bound + 2^-23): `bound` is the reference's own
sum, over the decays the row had taken, of |d ln f / du| * 1e-9 (1e-9: the project's bar for a device IoU against
eval_ref.iou_pair, tests/test_gpu_detection_eval.py), 2^-23 the one rounding to float32, which may land on either neighbour; a
row no decay touched matches by bits.  An equal pick order can only be asked for where the reference's own walk does not hang
on the last bits, so three guards are asserted ON THE REFERENCE ALONE, before the device is looked at:
  1  at every pick the best and the runner-up are an exact tie of two rows no decay has touched, or differ by more than 1e-6
     relative (three orders above the bound);
  2  no evaluated IoU > 0 lies within 1e-7 of iou_thres;
  3  no decayed score compared with min_score lies within 1e-6 relative of it.
No seed was replaced and no case left out; the smallest figures over the cases below: guard 1 6.8e-6 (seed 1, K = 1000), guard 2
8.5e-4 (3D, K = 4096), guard 3 1.5e-2 (seed 2, K = 64); no touched tie.

Pools: tta_ref.clustered_pools(seed, 1, B, K, [identity]) — 25 jittered candidates per object, scores in [0.3, 1)."""
import functools
import math

import numpy as np
import pytest
import torch

import soft_nms_ref as S
import tta_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDENT = [(1.0, 0.0, 1.0)]
CASES = [(1, 1, 1, 0), (64, 20, 3, 2), (257, 64, 2, 3), (1000, 64, 3, 1), (4096, 64, 1, 5)]          # (K, P, B, seed)
METHODS = {"hard": S.HARD, "linear": S.LINEAR, "gaussian": S.GAUSSIAN}
METRICS = {"bev": S.BEV, "3d": S.D3}
SIGMA, FLOOR = 0.5, 0.05


def _thres(method):
    return 0.1 if method == "hard" else 0.3


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _host(*ts):
    return [t.cpu().numpy() for t in ts]


@functools.lru_cache(maxsize=None)
def _pool(K, B, seed):
    """one clustered pool (B = 3: sample 1 is empty), on the host and on the device, and the pair cache its references share"""
    boxes, scores, counts = T.clustered_pools(seed, 1, B, K, IDENT)
    boxes, scores, counts = boxes[0], scores[0], counts[0].copy()
    if B == 3:
        counts[1] = 0
    return dict(boxes=boxes, scores=scores, counts=counts, dev=(_dev(boxes), _dev(scores), _dev(counts)),
                cache=[{} for _ in range(B)])


@functools.lru_cache(maxsize=None)
def _reference(K, P, B, seed, method, metric):
    p = _pool(K, B, seed)
    return [S.soft_nms(p["boxes"][b], p["scores"][b], p["counts"][b], METHODS[method], METRICS[metric], _thres(method), SIGMA, FLOOR, P,
                       p["cache"][b]) for b in range(B)]


def _run(dev, method, metric, P, floor=FLOOR, thres=None):
    from voxelnet_amd.predict import SoftNMS, soft_nms_device
    soft = SoftNMS(method=method, sigma=SIGMA, iou_thres=_thres(method) if thres is None else thres, metric=metric)
    return soft_nms_device(*dev, soft, P, min_score=floor)


def _check_padding(keep, ks, kc, P):
    for b in range(keep.shape[0]):
        assert 0 <= kc[b] <= P and (keep[b, kc[b]:] == -1).all() and not ks[b, kc[b]:].any()
        assert (keep[b, :kc[b]] >= 0).all() and len(set(keep[b, :kc[b]].tolist())) == kc[b]


# ------------------------------------------------------------------------------------------------- against the reference
def _check_against(refs, p, out, P, what):
    """the guards on the reference alone, first; then the device's result against it -> how many decayed rows were kept"""
    for b, r in enumerate(refs):
        print(f"{what} b {b}: kept {len(r['keep'])} gap1 {r['gap1']:.3g} ties {r['touched_ties']} gap2 {r['gap2']:.3g} "
              f"floor {r['floor_gap']:.3g} decays <= {max(r['decays'], default=0)} bound <= {max(r['bound'], default=0):.3g}")
        assert r["touched_ties"] == 0 and r["gap1"] > 1e-6, (b, r["gap1"], r["touched_ties"])
        assert r["gap2"] > 1e-7, (b, r["gap2"])
        assert r["floor_gap"] > 1e-6 and all(math.isfinite(v) for v in r["bound"]), (b, r["floor_gap"])
    B = len(refs)
    keep, ks, kc = _host(*out)
    assert keep.shape == (B, P) and ks.shape == (B, P) and kc.shape == (B,)
    assert keep.dtype == np.int32 and ks.dtype == np.float32 and kc.dtype == np.int32
    _check_padding(keep, ks, kc, P)
    decayed_kept = 0
    for b, r in enumerate(refs):
        n = len(r["keep"])
        assert kc[b] == n and keep[b, :n].tolist() == r["keep"], (b, kc[b], n)
        ref = np.array(r["w"], dtype=np.float64)
        tol = ref * (np.array(r["bound"]) + 2.0 ** -23)
        err = np.abs(ks[b, :n].astype(np.float64) - ref)
        print(f"   b {b}: largest |dev - ref| / tol {float((err / tol).max()) if n else 0.0:.3g}")
        assert (err <= tol).all(), (b, float((err / tol).max()))
        plain = np.array(r["decays"]) == 0
        assert np.array_equal(_u32(ks[b, :n][plain]), _u32(p["scores"][b][np.array(r["keep"], dtype=np.int64)[plain]])), b
        assert (np.diff(ks[b, :n]) <= 0).all(), b
        decayed_kept += int((~plain).sum())
    return decayed_kept


@pytest.mark.parametrize("metric", ["bev", "3d"])
@pytest.mark.parametrize("method", ["hard", "linear", "gaussian"])
@pytest.mark.parametrize("K, P, B, seed", CASES)
def test_soft_nms_matches_the_reference(K, P, B, seed, method, metric):
    refs = _reference(K, P, B, seed, method, metric)
    p = _pool(K, B, seed)
    out = _run(p["dev"], method, metric, P)
    decayed_kept = _check_against(refs, p, out, P, f"K {K} {method}/{metric}")
    if B == 3:
        assert int(out[2][1]) == 0          # the empty sample
    if (K, method) in ((257, "linear"), (257, "gaussian"), (1000, "linear"), (1000, "gaussian")):
        assert decayed_kept > 0          # decayed rows were picked again
    if K == 257 and method != "hard":
        assert all(len(r["keep"]) < P for r in refs)          # the walk stopped on min_score
    again = _run(p["dev"], method, metric, P)
    assert all(torch.equal(a.view(torch.int32), c.view(torch.int32)) for a, c in zip(out, again))          # two launches, the same bits


@pytest.mark.parametrize("method, metric", [("gaussian", "bev"), ("linear", "3d"), ("hard", "bev")])
def test_one_cluster_of_more_rows_than_the_workgroup_has_threads(method, metric):
    """2100 candidates of ONE object: every row is near every pick, so the list of near rows is filled more than once per pick
    (the kernel's list holds one entry per thread).  P = 4: the plain-Python reference clips 3 x 2099 pairs."""
    K, P = 2100, 4
    boxes, scores, counts = T.clustered_pools(4, 1, 1, K, IDENT, per=K)
    p = dict(boxes=boxes[0], scores=scores[0], counts=counts[0])
    assert int(counts[0, 0]) == K
    ref = S.soft_nms(p["boxes"][0], p["scores"][0], K, METHODS[method], METRICS[metric], _thres(method), SIGMA, FLOOR, P)
    out = _run((_dev(p["boxes"]), _dev(p["scores"]), _dev(p["counts"])), method, metric, P)
    decayed_kept = _check_against([ref], p, out, P, f"one cluster {method}/{metric}")
    assert decayed_kept == (0 if method == "hard" else P - 1) and len(ref["keep"]) == (1 if method == "hard" else P)


# ------------------------------------------------------------------------------------------------- hard = the greedy NMS
@pytest.mark.parametrize("K, P, B, seed", [c for c in CASES if c[0] in (64, 1000, 4096)])
def test_hard_mode_is_the_greedy_nms(K, P, B, seed):
    from voxelnet_amd.predict import gather_kept, nms_device
    p = _pool(K, B, seed)
    boxes, scores, counts = p["dev"]
    assert (np.diff(p["scores"], axis=1) <= 0).all()          # the pool's scores do not increase along the rows
    keep, ks, kc = _run(p["dev"], "hard", "bev", P, thres=0.1)
    gk, gc = nms_device(boxes, counts, "rotated", 0.1, P)
    assert torch.equal(keep, gk) and torch.equal(kc, gc) and int(kc.sum()) >= 2
    _, gs, _ = gather_kept(boxes, scores, gk, gc)
    assert torch.equal(ks.view(torch.int32), gs.view(torch.int32))          # its scores are the pool's


# ------------------------------------------------------------------------------------------------- the arg-max
def _separated(K=4096):
    """K boxes on an 8 m pitch: no pair is near, nothing decays"""
    rng = np.random.default_rng(11)
    ix, iy = np.divmod(np.arange(K), 64)
    return np.stack([8.0 * ix, 8.0 * iy - 250.0, np.full(K, -1.0), np.full(K, 1.5), np.full(K, 1.6), np.full(K, 3.9),
                     rng.uniform(-math.pi, math.pi, K)], axis=1).astype(np.float32)


TOP_ROWS = [0, 63, 64, 1023, 1024, 2047, 3072, 4095]          # lanes 0 / 63, waves 0 / 1 / 15, every register slot


@pytest.mark.parametrize("method", ["gaussian", "hard"])
def test_the_pick_order_follows_the_scores_not_the_rows(method):
    K, P = 4096, 64
    rng = np.random.default_rng(5)
    boxes = _separated(K)
    scores = (rng.permutation(K).astype(np.float32) + 1.0) / np.float32(8192.0)          # distinct, in (0, 0.5]
    scores[TOP_ROWS] = np.float32(0.5) + np.arange(len(TOP_ROWS), 0, -1, dtype=np.float32)[rng.permutation(len(TOP_ROWS))] / np.float32(32.0)
    assert len(set(scores.tolist())) == K
    counts = np.array([K], dtype=np.int32)
    keep, ks, kc = _host(*_run((_dev(boxes[None]), _dev(scores[None]), _dev(counts)), method, "bev", P, floor=0.0))
    want = np.argsort(-scores.astype(np.float64), kind="stable")[:P]
    assert kc[0] == P and keep[0].tolist() == want.tolist() and set(want[:8].tolist()) == set(TOP_ROWS)
    assert np.array_equal(_u32(ks[0]), _u32(scores[want]))
    # bit-equal scores across a wave boundary, a q boundary and two register slots of one thread: the smaller row first
    ties = scores.copy()
    for k, (lo, hi) in enumerate([(63, 64), (1023, 1024), (5, 2053), (3071, 3072), (100, 4095)]):
        ties[lo] = ties[hi] = np.float32(0.875) + np.float32(k) / np.float32(64.0)
    keep, ks, kc = _host(*_run((_dev(boxes[None]), _dev(ties[None]), _dev(counts)), method, "bev", P, floor=0.0))
    want = np.lexsort((np.arange(K), -ties.astype(np.float64)))[:P]
    assert want[:10].tolist() == [100, 4095, 3071, 3072, 5, 2053, 1023, 1024, 63, 64]
    assert kc[0] == P and keep[0].tolist() == want.tolist() and np.array_equal(_u32(ks[0]), _u32(ties[want]))


@pytest.mark.parametrize("method, metric", [("gaussian", "bev"), ("linear", "3d"), ("hard", "bev")])
def test_a_permutation_of_the_rows_keeps_the_same_boxes(method, metric):
    K, P, B, seed = 1000, 64, 3, 1
    p = _pool(K, B, seed)
    boxes, scores, n = p["boxes"][0], p["scores"][0], int(p["counts"][0])
    assert len(set(scores[:n].tolist())) == n          # distinct scores: the pick order does not depend on the rows
    perm = np.random.default_rng(3).permutation(n)
    pb, ps = boxes.copy(), scores.copy()
    pb[:n], ps[:n] = boxes[perm], scores[perm]
    cnt = np.array([n], dtype=np.int32)
    a = _host(*_run((_dev(boxes[None]), _dev(scores[None]), _dev(cnt)), method, metric, P))
    c = _host(*_run((_dev(pb[None]), _dev(ps[None]), _dev(cnt)), method, metric, P))
    m = int(a[2][0])
    assert m == c[2][0] and m > 0
    assert perm[c[0][0, :m]].tolist() == a[0][0, :m].tolist()          # the same rows, in the same order
    assert np.array_equal(_u32(a[1]), _u32(c[1]))          # with the same scores: the product order is the pick order


# ------------------------------------------------------------------------------------------------- edges
def test_counts_outside_the_pool_are_clamped():
    K, P = 64, 20
    p = _pool(K, 3, 2)
    boxes, scores = p["dev"][0], p["dev"][1]
    n = int(p["counts"][0])
    full = _run((boxes, scores, _dev(np.array([n, n, n], dtype=np.int32))), "gaussian", "bev", P)
    odd = _run((boxes, scores, _dev(np.array([K + 5, -3, n], dtype=np.int32))), "gaussian", "bev", P)
    assert n <= K and int(odd[2][1]) == 0 and (odd[0][1] == -1).all() and not odd[1][1].any()
    assert torch.equal(odd[0][2], full[0][2]) and torch.equal(odd[1][2], full[1][2])
    # rows n .. K-1 of the pool are zero boxes (l = 0): a count above K walks K rows and never keeps one of them
    assert torch.equal(odd[0][0], full[0][0]) and torch.equal(odd[1][0].view(torch.int32), full[1][0].view(torch.int32))


@pytest.mark.parametrize("method", ["hard", "linear", "gaussian"])
def test_ineligible_rows_are_never_kept_and_decay_nothing(method):
    """a row with a NaN field, a row with l = 0, a NaN score and a +inf score, each a copy of the best row of a cluster: the result
    is the one of the pool without them"""
    K, P = 257, 64
    p = _pool(K, 2, 3)
    boxes, scores, n = p["boxes"][0], p["scores"][0], int(p["counts"][0])
    clean_b, clean_s = boxes[:n], scores[:n]
    top = clean_b[0]
    bad_b = np.stack([top, top, top, top]).copy()
    bad_s = np.array([2.0, 3.0, np.nan, np.inf], dtype=np.float32)          # above every score: they would be picked first
    bad_b[0, 1], bad_b[1, 5] = np.nan, 0.0
    at = [0, 70, 130, n + 3]          # where they go in the dirty pool
    db, ds, src = [], [], []
    it = iter(range(n))
    for pos in range(n + 4):
        if pos in at:
            k = at.index(pos)
            db.append(bad_b[k]), ds.append(bad_s[k]), src.append(-1)
        else:
            j = next(it)
            db.append(clean_b[j]), ds.append(clean_s[j]), src.append(j)
    db, ds, src = np.array(db, dtype=np.float32), np.array(ds, dtype=np.float32), np.array(src)
    a = _host(*_run((_dev(clean_b[None]), _dev(clean_s[None]), _dev(np.array([n], dtype=np.int32))), method, "bev", P))
    c = _host(*_run((_dev(db[None]), _dev(ds[None]), _dev(np.array([n + 4], dtype=np.int32))), method, "bev", P))
    m = int(a[2][0])
    assert m == c[2][0] and m > 2
    assert src[c[0][0, :m]].tolist() == a[0][0, :m].tolist() and np.array_equal(_u32(a[1]), _u32(c[1]))


def test_min_score_top_k_one_and_repeat():
    K, P = 257, 64
    p = _pool(K, 2, 3)
    keep, ks, kc = _run(p["dev"], "gaussian", "bev", P, floor=1.5)          # above every score
    assert kc.tolist() == [0, 0] and (keep == -1).all() and not ks.any()
    keep, ks, kc = _host(*_run(p["dev"], "linear", "3d", 1))
    best = p["scores"].argmax(axis=1)
    assert kc.tolist() == [1, 1] and keep[:, 0].tolist() == best.tolist()
    assert np.array_equal(_u32(ks[:, 0]), _u32(p["scores"][np.arange(2), best]))
    # a floor between the scores: exactly the rows at or above it under "hard" with a threshold that removes nothing
    floor = float(np.float32(0.9))
    keep, ks, kc = _host(*_run(p["dev"], "hard", "bev", P, floor=floor, thres=1.0))
    for b in range(2):
        assert kc[b] == min(P, int((p["scores"][b] >= np.float32(floor)).sum())) and (ks[b, :kc[b]] >= np.float32(floor)).all()


# ------------------------------------------------------------------------------------------------- composition
HEADS = [dict(), dict(dir_head=True, iou_head=True, anchor_area_threshold=1)]
SOFT_DECODE = dict(score_thres=1e-6, nms="rotated", nms_thres=0.1, pre_nms_top_k=96, layout="site")


@pytest.mark.parametrize("heads", HEADS, ids=["plain", "dir+iou+mask"])
def test_decode_device_soft_nms_is_the_chain_of_its_pieces(heads):
    import test_gpu_tta as G
    from voxelnet_amd import model as M
    from voxelnet_amd import tta
    from voxelnet_amd.predict import BoxDecoder, SoftNMS, gather_kept, soft_nms_device
    from voxelnet_amd.targets import generate_anchors
    before = M.get_precision()
    M.set_precision("bf16")
    try:
        m = G._tiny_model(**heads).eval()
        x = G._tiny_batches((tta.View(),))[0]
        dec = BoxDecoder("Car", DEV, anchors=generate_anchors("Car")[:8, :12])
        with torch.no_grad():
            prob, delta = m.detect(x[2], x[4])
        kw = m._dir_decode(dict(layout="site"), dec)
        if heads:
            kw["anchor_mask"] = m._decode_mask(dec, x[4], torch.device(DEV))
        for soft in (SoftNMS(), SoftNMS(method="linear", metric="3d", min_score=1e-3)):
            got = dec.decode_device(prob, delta, score_thres=1e-6, nms_thres=0.1, top_k=20, nms="rotated", pre_nms_top_k=96, soft_nms=soft, **kw)
            cb, cs, idx, cc = dec.candidates_device(prob, delta, 1e-6, 96, **kw)
            keep, ks, kc = soft_nms_device(cb, cs, cc, soft, 20, min_score=1e-6)
            want = gather_kept(cb, cs, keep, kc, keep_scores=ks)
            for a, b in zip(got, want):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            assert int(got[2].sum()) > 0 and (got[1][:, :-1] >= got[1][:, 1:]).all()
            # nms_thres is not read
            other = dec.decode_device(prob, delta, score_thres=1e-6, nms_thres=0.9, top_k=20, nms="rotated", pre_nms_top_k=96, soft_nms=soft, **kw)
            assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, other))
        live = torch.arange(20, device=DEV)[None, :] < kc[:, None]
        assert ((want[1] < torch.gather(cs, 1, keep.clamp(min=0).long())) & live).any()          # a decayed row was kept all the same
        lb, ls = dec(prob, delta, score_thres=1e-6, nms_thres=0.1, top_k=20, nms="rotated", pre_nms_top_k=96, soft_nms=soft, **kw)
        assert [len(s) for s in ls] == got[2].tolist() and np.array_equal(lb[0], got[0][0, :len(lb[0])].cpu().numpy())
        assert np.array_equal(ls[0], got[1][0, :len(ls[0])].cpu().numpy())
        with pytest.raises(ValueError, match="vote"):
            dec.decode_device(prob, delta, score_thres=1e-6, top_k=20, nms="rotated", pre_nms_top_k=96, soft_nms=soft, vote=tta.BoxVote(), **kw)
        with pytest.raises(ValueError, match="rotated"):
            dec.decode_device(prob, delta, score_thres=1e-6, top_k=20, nms="standup", pre_nms_top_k=96, soft_nms=soft, **kw)
        with pytest.raises(ValueError, match="SoftNMS"):
            dec.decode_device(prob, delta, score_thres=1e-6, top_k=20, nms="rotated", pre_nms_top_k=96, soft_nms="gaussian", **kw)
    finally:
        M.set_precision(before)


@pytest.mark.parametrize("heads", HEADS, ids=["plain", "dir+iou+mask"])
def test_evaluate_and_predict_with_soft_nms_are_the_pipeline_written_out(heads):
    import test_gpu_tta as G
    from voxelnet_amd import model as M
    from voxelnet_amd import tta
    from voxelnet_amd.evaluate import DetectionEvaluator
    from voxelnet_amd.predict import BoxDecoder, SoftNMS, gather_kept, soft_nms_device
    from voxelnet_amd.targets import generate_anchors
    views = (tta.View(), tta.View(flip_y=True))
    aug = tta.TestTimeAugment(views=views, vote=None)
    soft = SoftNMS()
    decode = dict(SOFT_DECODE, soft_nms=soft)
    before = M.get_precision()
    M.set_precision("bf16")
    try:
        m = G._tiny_model(**heads)
        batches = G._tiny_batches(views)
        dec = BoxDecoder("Car", DEV, anchors=generate_anchors("Car")[:8, :12])
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        got = m.evaluate(batches, DEV, decoder=dec, decode=decode)
        got_tta = m.evaluate(batches, DEV, decoder=dec, decode=decode, tta=aug)
        assert m.training and all(mod.training for mod in m.modules())
        for k, v in m.state_dict().items():          # mode, parameters, running statistics: untouched
            assert torch.equal(v, state[k]), k
        with pytest.raises(ValueError, match="vote=None"):
            m.evaluate(batches, DEV, decoder=dec, decode=decode, tta=tta.TestTimeAugment(views=views))
        with pytest.raises(ValueError, match="rotated"):
            m.evaluate(batches, DEV, decoder=dec, decode=dict(decode, nms="standup"), tta=aug)
        with pytest.raises(ValueError, match="rotated"):
            m.evaluate(batches, DEV, decoder=dec, decode=dict(decode, nms="standup"))
        with pytest.raises(ValueError, match="vote"):
            m.evaluate(batches, DEV, decoder=dec, decode=dict(decode, vote=tta.BoxVote()))
        assert m.training
        # ---- the same two pipelines from the public pieces
        want, want_tta = DetectionEvaluator("Car", DEV), DetectionEvaluator("Car", DEV)
        m.eval()
        hand, hand_tta = [], []
        with torch.no_grad():
            for x in batches:
                pools = []
                for view in views:
                    if view.identity:
                        feats, coords = x[2], x[4]
                    else:
                        from voxelnet_amd.voxelize import voxelize_device
                        feats, coords = [], []
                        for b, raw in enumerate(x[6]):
                            pts, _ = aug.view_points(view, raw, x[0][b], None, torch.device(DEV))
                            fb, cb, _ = voxelize_device(pts, m.feature_net._grid, b, coord_cols=4)
                            feats.append(fb)
                            coords.append(cb)
                    prob, delta = m.detect(feats, coords)
                    kw = m._dir_decode(dict(layout="site"), dec)
                    if heads:
                        kw["anchor_mask"] = m._decode_mask(dec, coords, torch.device(DEV))
                    pools.append(dec.candidates_device(prob, delta, 1e-6, 96, **kw))
                cb, cs, _, cc = pools[0]
                keep, ks, kc = soft_nms_device(cb, cs, cc, soft, want.top_k, min_score=1e-6)
                det = gather_kept(cb, cs, keep, kc, keep_scores=ks)
                want.update(*det, x[1])
                hand.append(det)
                mb, ms, src, mc = tta.merge_pools([p[0] for p in pools], [p[1] for p in pools], [p[3] for p in pools], views)
                keep, ks, kc = soft_nms_device(mb, ms, mc, soft, want.top_k, min_score=1e-6)
                det = gather_kept(mb, ms, keep, kc, keep_scores=ks)
                want_tta.update(*det, x[1])
                hand_tta.append(det)
            m.__dict__["_decoder"] = dec
            prob, delta = m.detect(batches[0][2], batches[0][4])
            _, rows = m.predict(batches[0], prob, delta, decode=dict(decode, top_k=want.top_k))
            _, rows_tta = m.predict(batches[0], prob, delta, decode=dict(decode, top_k=want.top_k), tta=aug)
        G._same_metrics(got.compute(), want.compute())
        G._same_metrics(got_tta.compute(), want_tta.compute())
        assert got.compute()["n_det"] > 0 and got_tta.compute()["n_det"] > 0
        assert int(hand_tta[0][2].sum()) > 0 and not torch.equal(hand[0][1], hand_tta[0][1])          # the merged pool is another pool
        for rws, h in ((rows, hand[0]), (rows_tta, hand_tta[0])):
            hb, hs, hc = _host(*h)
            for b in range(2):
                assert len(rws[b]) == hc[b]
                assert np.allclose(rws[b][:, 1:8].astype(np.float64), hb[b, :hc[b]], rtol=1e-6, atol=0)          # (via strings)
                assert np.allclose(rws[b][:, 8].astype(np.float64), hs[b, :hc[b]], rtol=1e-6, atol=0)
    finally:
        M.set_precision(before)
