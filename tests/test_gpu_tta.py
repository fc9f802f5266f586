"""GPU: test-time augmentation and box voting (csrc/tta.hip through vn_pool_merge / vn_box_vote, voxelnet_amd/tta.py, the
vote= / tta= keywords) against the float64 restatement tests/tta_ref.py.

Bars.  Merge: counts, order, src and scores bit-exact; boxes within the project's decode bar (rtol 2.4e-7, atol 1e-6, the one of
tests/test_gpu_predict.py: the device rounds a float64 result to float32 once, the host's cos / sin may differ from NumPy's in
the last bit); the identity view bit for bit.  Vote: the reference walks THE DEVICE'S OWN merged float32 pool and kept rows, read
back, so a last-bit difference of the merge cannot flip a membership; the test first asserts ON THE REFERENCE ALONE that no
IoU > 0 it evaluated lies within 1e-7 of vote_thres (two orders above the 1e-9 device / reference agreement of the pair
function) and that no member's |d| lies within 1e-6 of pi/2; then out_members, out_counts, the row order and
the scores must be equal exactly and the fields within the same float32 bar.  No seed had to be replaced: seeds 1-3 hold both
guards in every case below.

Clustered scenes (tta_ref.clustered_pools): objects on a 6 m pitch, 25 jittered candidates per object and view, every third
turned by pi, seen through each view; merged, suppressed by nms_device at 0.1, voted at 0.5 and 0.7."""
import functools
import math
from dataclasses import replace

import numpy as np
import pytest
import torch

import tta_ref as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 2.4e-7, 1e-6
VIEWS8 = [(1.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (1.0, math.pi / 8, float(np.float32(1.05))), (-1.0, -0.3, float(np.float32(0.95))),
          (1.0, 3.0, 1.0), (-1.0, 1.0, 2.0), (1.0, -2.5, 0.5), (1.0, 0.0, 1.0)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _host(*ts):
    return [t.cpu().numpy() for t in ts]


# ------------------------------------------------------------------------------------------------------- merge
def _merge_inputs(V, B, K):
    """random boxes in view coordinates; scores on a grid of 48 values (ties inside a view and across views) with zeros of
    both signs and a NaN in every view; counts cycle through 0, a partial pool, a value above K and K"""
    rng = np.random.default_rng(100 * V + 10 * B + K)
    boxes = np.concatenate([rng.uniform(-60, 60, (V, B, K, 3)), rng.uniform(0.5, 4.5, (V, B, K, 3)),
                            rng.uniform(-4, 4, (V, B, K, 1))], axis=3).astype(np.float32)
    scores = (rng.integers(1, 49, (V, B, K)) / 64.0).astype(np.float32)
    if K >= 8:
        scores[:, :, 1], scores[:, :, 3], scores[:, :, 4], scores[:, :, 6] = 0.0, -0.0, np.nan, scores[:, :, 0]
    cyc = [0, K // 2, K + 5, K]
    counts = np.array([[cyc[(v + 2 * b + 1) % 4] for b in range(B)] for v in range(V)], dtype=np.int32)
    if K == 1:
        counts[:] = 1
    return boxes, scores, counts, np.array(VIEWS8[:V], dtype=np.float64)


@pytest.mark.parametrize("V, B, K", [(1, 1, 1), (2, 3, 63), (4, 2, 65), (3, 2, 257), (4, 2, 1024), (8, 1, 512)])
def test_merge_matches_the_reference(V, B, K):
    from voxelnet_amd import tta
    boxes, scores, counts, views = _merge_inputs(V, B, K)
    out = tta.merge_pools(_dev(boxes), _dev(scores), _dev(counts), views)
    again = tta.merge_pools([_dev(boxes[v]) for v in range(V)], [_dev(scores[v]) for v in range(V)],
                            [_dev(counts[v]) for v in range(V)], views)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, again))          # lists = stacked; same bits
    ob, os_, src, oc = _host(*out)
    assert ob.shape == (B, V * K, 7) and os_.shape == (B, V * K) and src.dtype == np.int32 and oc.dtype == np.int32
    assert K == 1 or (counts == 0).any() and (counts > K).any() and ((counts > 0) & (counts < K)).any()
    for b in range(B):
        rb, rs, rsrc = T.merge(boxes[:, b], scores[:, b], counts[:, b], views)
        n = len(rs)
        assert oc[b] == n and np.array_equal(src[b, :n], rsrc), b
        assert np.array_equal(_u32(os_[b, :n]), _u32(rs)), b
        assert np.allclose(ob[b, :n], rb, rtol=RTOL, atol=ATOL), np.abs(ob[b, :n] - rb).max()
        assert not ob[b, n:].any() and not os_[b, n:].any() and not src[b, n:].any()          # zero-filled by the wrapper
        ident = np.isin(rsrc // K, [v for v in range(V) if tuple(views[v]) == (1.0, 0.0, 1.0)])
        assert np.array_equal(_u32(ob[b, :n][ident]), _u32(boxes[:, b].reshape(V * K, 7)[rsrc[ident]])), b
        assert K < 8 or (np.diff(os_[b, :n]) == 0).any()          # the case has ties to order


def test_merge_identity_view_passes_through():
    from voxelnet_amd import tta
    boxes, scores, _, _ = _merge_inputs(1, 2, 300)
    scores = np.sort(np.nan_to_num(scores, nan=0.5), axis=2)[:, :, ::-1].copy()          # a pool as candidates_device makes it
    counts = np.array([[300, 123]], dtype=np.int32)
    ob, os_, src, oc = tta.merge_pools(_dev(boxes), _dev(scores), _dev(counts), (tta.View(),))
    assert oc.tolist() == [300, 123]
    for b, n in enumerate((300, 123)):
        assert torch.equal(ob[b, :n], _dev(boxes[0, b, :n])) and torch.equal(os_[b, :n], _dev(scores[0, b, :n]))
        assert src[b, :n].tolist() == list(range(n))          # equal scores keep their order: the smaller src first


# ------------------------------------------------------------------------------------------------------- vote
# (K rows of the merged pool, P kept rows, V views, B samples, vote_thres, weight, score, seed)
VOTE_CASES = [(1, 1, 1, 1, 0.5, "score_iou", "keep", 1),
              (64, 20, 1, 3, 0.5, "score", "keep", 2),
              (257, 20, 4, 1, 0.7, "score_iou", "view_mean", 3),
              (1000, 64, 4, 3, 0.5, "score_iou", "view_mean", 1),
              (1000, 20, 1, 3, 0.7, "score", "view_mean", 2),
              (4096, 64, 4, 1, 0.7, "score", "view_mean", 2),
              (4096, 64, 1, 1, 0.5, "score_iou", "keep", 3)]


@functools.lru_cache(maxsize=None)
def _pool(K, P, V, B, seed):
    """the device's merged pool of a clustered scene, cut to K rows, and nms_device's kept rows on it (B = 3: sample 1 is empty)"""
    from voxelnet_amd import tta
    from voxelnet_amd.predict import nms_device
    Kv = -(-K // V)
    views = np.array(VIEWS8[:V], dtype=np.float64)
    boxes, scores, counts = T.clustered_pools(seed, V, B, Kv, views)
    if B == 3:
        counts[:, 1] = 0
    mb, ms, src, mc = tta.merge_pools(_dev(boxes), _dev(scores), _dev(counts), views)
    mb, ms, src, mc = mb[:, :K].contiguous(), ms[:, :K].contiguous(), src[:, :K].contiguous(), mc.clamp(max=K)
    keep, kc = nms_device(mb, mc, "rotated", 0.1, P)
    return dict(mb=mb, ms=ms, src=src, mc=mc, keep=keep, kc=kc, Kv=Kv, host=_host(mb, ms, src, mc, keep, kc))


def _check_vote(p, out, V, P, thres, weight, score, keep_counts=None):
    from voxelnet_amd import tta
    mb, ms, src, mc, keep, kc = p["host"]
    kc = kc if keep_counts is None else keep_counts
    ob, os_, oc, om = _host(*out)
    wm, sm = tta.WEIGHTS[weight], tta.SCORES[score]
    assert (wm, sm) == ({"score": T.W_SCORE, "score_iou": T.W_SCORE_IOU}[weight], {"keep": T.S_KEEP, "view_mean": T.S_VIEW_MEAN}[score])
    members_seen = 0
    for b in range(mb.shape[0]):
        ref = T.vote(mb[b], ms[b], mc[b], keep[b, :kc[b]], thres, wm, sm, src=src[b], rows_per_view=p["Kv"], V=V)
        assert ref["iou_gap"] > 1e-7 and ref["wrap_gap"] > 1e-6, (b, ref["iou_gap"], ref["wrap_gap"])          # the guards, first
        n = len(ref["scores"])
        assert n == kc[b] and oc[b] == n, b
        assert np.array_equal(om[b, :n], ref["members"]), b
        assert np.array_equal(_u32(os_[b, :n]), _u32(ref["scores"])), b
        assert np.allclose(ob[b, :n], ref["boxes"].astype(np.float32), rtol=RTOL, atol=ATOL), b
        assert not ob[b, n:].any() and not os_[b, n:].any() and not om[b, n:].any()
        members_seen = max(members_seen, int(ref["members"].max()) if n else 0)
    return members_seen


@pytest.mark.parametrize("K, P, V, B, thres, weight, score, seed", VOTE_CASES)
def test_vote_matches_the_reference(K, P, V, B, thres, weight, score, seed):
    from voxelnet_amd import tta
    p = _pool(K, P, V, B, seed)
    vote = tta.BoxVote(thres=thres, weight=weight, score=score)
    kw = dict(src=p["src"], rows_per_view=p["Kv"], n_views=V)
    out = tta.vote_device(p["mb"], p["ms"], p["mc"], p["keep"], p["kc"], vote, **kw)
    seen = _check_vote(p, out, V, P, thres, weight, score)
    assert K < 64 or seen > 1          # clusters were fused, not only copied
    again = tta.vote_device(p["mb"], p["ms"], p["mc"], p["keep"], p["kc"], vote, **kw)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, again))          # two launches, the same bits
    if V == 1:          # without src every row is view 0: the same result
        plain = tta.vote_device(p["mb"], p["ms"], p["mc"], p["keep"], p["kc"], vote)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, plain))
    if B == 3:
        assert out[2].tolist()[1] == 0 and p["kc"].tolist()[1] == 0          # the empty sample


@pytest.mark.parametrize("K, P, V, B, seed", [(64, 20, 1, 3, 2), (1000, 64, 4, 3, 1)])
def test_vote_above_one_returns_the_kept_rows(K, P, V, B, seed):
    """vote_thres = 2.0: no member but the row itself — the kept rows bit for bit, in the walk order"""
    from voxelnet_amd import tta
    from voxelnet_amd.predict import gather_kept
    p = _pool(K, P, V, B, seed)
    for weight in ("score", "score_iou"):
        ob, os_, oc, om = tta.vote_device(p["mb"], p["ms"], p["mc"], p["keep"], p["kc"], tta.BoxVote(thres=2.0, weight=weight),
                                          src=p["src"], rows_per_view=p["Kv"], n_views=V)
        gb, gs, gc = gather_kept(p["mb"], p["ms"], p["keep"], p["kc"])
        assert torch.equal(oc, gc) and torch.equal(ob.view(torch.int32), gb.view(torch.int32))
        assert torch.equal(os_.view(torch.int32), gs.view(torch.int32))
        live = torch.arange(P, device=DEV)[None, :] < oc[:, None]
        assert torch.equal(om, live.to(torch.int32)) and int(oc.sum()) > 0


def test_vote_with_a_keep_count_of_zero():
    from voxelnet_amd import tta
    K, P, V, B, seed = 64, 20, 1, 3, 2
    p = _pool(K, P, V, B, seed)
    kc = p["kc"].clone()
    kc[2] = 0
    out = tta.vote_device(p["mb"], p["ms"], p["mc"], p["keep"], kc, tta.BoxVote(), src=p["src"], rows_per_view=p["Kv"], n_views=V)
    assert out[2].tolist()[1:] == [0, 0] and out[2].tolist()[0] > 0
    _check_vote(p, out, V, P, 0.5, "score_iou", "keep", keep_counts=kc.cpu().numpy())


def test_vote_skips_entries_the_nms_never_writes():
    """a keep_idx outside the pool and an invalid kept row are skipped; the remaining rows close up"""
    from voxelnet_amd import tta
    p = _pool(64, 20, 1, 3, 2)
    keep, kc = p["keep"].clone(), p["kc"].clone()
    n0 = int(kc[0])
    assert n0 >= 2
    keep[0, 0] = 4000
    out = tta.vote_device(p["mb"], p["ms"], p["mc"], keep, kc, tta.BoxVote(), src=p["src"], rows_per_view=p["Kv"], n_views=1)
    mb, ms, src, mc = p["host"][:4]
    ref = T.vote(mb[0], ms[0], mc[0], keep[0, :n0].cpu().numpy(), 0.5, T.W_SCORE_IOU, T.S_KEEP)
    assert out[2].tolist()[0] == n0 - 1 == len(ref["scores"])
    assert np.array_equal(_u32(out[1][0, :n0 - 1].cpu().numpy()), _u32(ref["scores"]))
    assert np.array_equal(out[3][0, :n0 - 1].cpu().numpy(), ref["members"])


# ------------------------------------------------------------------------------------------------------- composition
def _tiny_grid():
    from voxelnet_amd.config import grid_config
    return replace(grid_config("Car"), H=16, W=24)


def _view_inverse_points(cloud, view):
    """the cloud that `view` maps onto `cloud` (float64, rounded once): every view of the union below has points on the grid"""
    fy, angle, f = view.row()
    q = cloud.astype(np.float64).copy()
    q[:, :3] /= f
    c, s = math.cos(angle), math.sin(angle)
    x, y = q[:, 0] * c - q[:, 1] * s, q[:, 0] * s + q[:, 1] * c
    q[:, 0], q[:, 1] = x, fy * y
    return q.astype(np.float32)


def _tiny_batches(views):
    """test_gpu_detection_eval.py::test_rpn3d_evaluate_runs_the_loop's batches on the tiny grid, with raw clouds in x[6]: each
    raw cloud is the union of a synthetic cloud's pre-images under every view, and x[2] / x[4] are its voxels"""
    from voxelnet_amd import synth
    from voxelnet_amd.voxelize import voxelize_device
    g = _tiny_grid()
    batches = []
    for k in range(2):
        feats, coords, raws = [], [], []
        for b in range(2):
            cloud = synth.synth_cloud("Car", k0=150 + 40 * b, seed=500 + 10 * k + b, grid=g, overflow_frac=0.03)
            raw = np.concatenate([_view_inverse_points(cloud, v) for v in views])
            fb, cb, _ = voxelize_device(torch.from_numpy(raw).to(DEV), g, b, coord_cols=4)
            feats.append(fb)
            coords.append(cb)
            raws.append(raw)
        labels = [synth.synth_labels("Car", 3, 40 + 2 * k + b) for b in range(2)]
        batches.append(([f"{2 * k + b:06d}" for b in range(2)], labels, feats, None, coords, None, raws))
    return batches


def _tiny_model(**kw):
    from oracle import torch_ref as tr
    from voxelnet_amd import model as M
    torch.manual_seed(7)
    m = M.RPN3D("Car", **kw)
    res = m.load_state_dict(tr.make_state_dict("Car"), strict=False)
    assert all("dir_conv" in k or "iou_conv" in k for k in res.missing_keys) and not res.unexpected_keys
    m.feature_net._grid = _tiny_grid()
    return m.to(DEV).train()


def _same_metrics(a, b):
    np.testing.assert_equal(a, b)          # (NaN == NaN here: an AP without ground truth)


HEADS = [dict(), dict(dir_head=True, iou_head=True, anchor_area_threshold=1)]


@pytest.mark.parametrize("heads", HEADS, ids=["plain", "dir+iou+mask"])
def test_decode_device_vote_is_the_chain_of_its_three_calls(heads):
    from voxelnet_amd import model as M
    from voxelnet_amd import tta
    from voxelnet_amd.predict import BoxDecoder, nms_device
    from voxelnet_amd.targets import generate_anchors
    before = M.get_precision()
    M.set_precision("bf16")
    try:
        m = _tiny_model(**heads).eval()
        x = _tiny_batches((tta.View(),))[0]
        dec = BoxDecoder("Car", DEV, anchors=generate_anchors("Car")[:8, :12])
        with torch.no_grad():
            prob, delta = m.detect(x[2], x[4])
        kw = m._dir_decode(dict(layout="site"), dec)
        if heads:
            kw["anchor_mask"] = m._decode_mask(dec, x[4], torch.device(DEV))
        vote = tta.BoxVote()
        got = dec.decode_device(prob, delta, score_thres=1e-6, nms_thres=0.1, top_k=20, nms="rotated", pre_nms_top_k=96, vote=vote, **kw)
        cb, cs, idx, cc = dec.candidates_device(prob, delta, 1e-6, 96, **kw)
        keep, kc = nms_device(cb, cc, "rotated", 0.1, 20)
        want = tta.vote_device(cb, cs, cc, keep, kc, vote)
        for a, b in zip(got, want[:3]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert int(got[2].sum()) > 0 and int(want[3].max()) > 1          # something was fused
        plain = dec.decode_device(prob, delta, score_thres=1e-6, nms_thres=0.1, top_k=20, nms="rotated", pre_nms_top_k=96, **kw)
        assert torch.equal(plain[2], got[2]) and not torch.equal(plain[0], got[0])          # the same kept set, other boxes
        lb, ls = dec(prob, delta, score_thres=1e-6, nms_thres=0.1, top_k=20, nms="rotated", pre_nms_top_k=96, vote=vote, **kw)
        assert [len(s) for s in ls] == got[2].tolist() and np.array_equal(lb[0], got[0][0, :len(lb[0])].cpu().numpy())
    finally:
        M.set_precision(before)


def test_evaluate_with_the_identity_view_alone_is_the_plain_evaluate():
    from voxelnet_amd import model as M
    from voxelnet_amd import tta
    from voxelnet_amd.predict import BoxDecoder
    from voxelnet_amd.targets import generate_anchors
    before = M.get_precision()
    M.set_precision("bf16")
    try:
        m = _tiny_model()
        batches = _tiny_batches((tta.View(),))
        dec = BoxDecoder("Car", DEV, anchors=generate_anchors("Car")[:8, :12])
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        only = tta.TestTimeAugment(views=(tta.View(),), vote=None)
        for decode in (None, dict(score_thres=1e-6, nms="rotated", nms_thres=0.1, pre_nms_top_k=96, layout="site")):
            plain = m.evaluate(batches, DEV, decoder=dec, decode=decode).compute()
            _same_metrics(m.evaluate(batches, DEV, decoder=dec, decode=decode, tta=only).compute(), plain)
            assert m.training and all(mod.training for mod in m.modules())
        assert plain["n_det"] > 0 and plain["n_gt"]["all"] == 12
        for k, v in m.state_dict().items():
            assert torch.equal(v, state[k]), k
        from voxelnet_amd import _lib
        with pytest.raises(_lib.VoxelnetHipError, match="raw"):
            m.evaluate([b[:6] + (None,) for b in batches], DEV, decoder=dec, tta=tta.TestTimeAugment())
        with pytest.raises(ValueError, match="4096"):
            m.evaluate(batches, DEV, decoder=dec, decode=dict(pre_nms_top_k=2049), tta=tta.TestTimeAugment())
    finally:
        M.set_precision(before)


def test_view_points_crops_and_moves_like_the_input_pipeline(golden, tmp_path):
    """TestTimeAugment(fov_calib_dir=).view_points: upload, the padded field-of-view crop of DeviceCollate (NaN rows past the
    count), then the view's affine — the oracle's crop moved in float64 on the host"""
    import os

    from oracle import fov as of
    from voxelnet_amd import augment as A
    from voxelnet_amd import tta
    g = golden("fov_crop")
    rows, cols = (int(v) for v in g["image_shape"])
    calib = tmp_path / "calib"
    calib.mkdir()

    def fmt(name, a):
        return name + ": " + " ".join(f"{v:.12e}" for v in np.asarray(a).reshape(-1))
    (calib / "000007.txt").write_text("\n".join([fmt("P0", g["P"]), fmt("P1", g["P"]), fmt("P2", g["P"]), fmt("P3", g["P"]),
                                                 fmt("R0_rect", g["R"][:3, :3]), fmt("Tr_velo_to_cam", g["Tr"][:3]),
                                                 fmt("Tr_imu_to_velo", g["Tr"][:3])]) + "\n")
    rng = np.random.default_rng(9)
    cloud = np.stack([rng.uniform(0, 70, 20000), rng.uniform(-40, 40, 20000), rng.uniform(-3, 1, 20000), rng.uniform(0, 1, 20000),
                      np.zeros(20000)], 1).astype(np.float32)          # a fifth column: only [:, :4] travels
    view = tta.View(flip_y=True, angle=0.2, scale=1.05)
    aug = tta.TestTimeAugment(views=(tta.View(), view), fov_calib_dir=str(calib), image_shape=(rows, cols))
    pts, _ = aug.view_points(view, cloud, "000007", None, torch.device(DEV))
    got = pts.cpu().numpy()
    live = ~np.isnan(got[:, 0])
    from voxelnet_amd.fov import load_calib
    P, Tr, R = load_calib(os.path.join(str(calib), "000007.txt"))
    cropped, _ = of.fov_crop(np.ascontiguousarray(cloud[:, :4]), P, Tr, R, rows, cols)
    assert got.shape == (20000, 4) and 0 < len(cropped) < 20000 and live.sum() == len(cropped) and live[:len(cropped)].all()
    a = A.compose_affine(True, 0.2, 1.05, None)
    c = cropped.astype(np.float64)
    want = np.stack([a[0] * c[:, 0] + a[1] * c[:, 1], a[2] * c[:, 0] + a[3] * c[:, 1], a[4] * c[:, 2], c[:, 3]], 1)
    assert np.allclose(got[live], want, rtol=1e-6, atol=1e-6) and np.array_equal(got[live][:, 3], cropped[:, 3])


@pytest.mark.parametrize("heads", HEADS, ids=["plain", "dir+iou+mask"])
def test_evaluate_with_three_views_is_the_pipeline_written_out(heads):
    from voxelnet_amd import augment as A
    from voxelnet_amd import model as M
    from voxelnet_amd import tta
    from voxelnet_amd.evaluate import DetectionEvaluator
    from voxelnet_amd.model import _batch_cat
    from voxelnet_amd.predict import BoxDecoder, nms_device
    from voxelnet_amd.targets import generate_anchors
    from voxelnet_amd.voxelize import voxelize_device
    views = (tta.View(), tta.View(flip_y=True), tta.View(angle=math.pi / 8, scale=1.05))
    vote = tta.BoxVote(score="view_mean")
    aug = tta.TestTimeAugment(views=views, vote=vote)
    decode = dict(score_thres=1e-6, nms="rotated", nms_thres=0.1, pre_nms_top_k=96, layout="site")
    before = M.get_precision()
    M.set_precision("bf16")
    try:
        m = _tiny_model(**heads)
        g = m.feature_net._grid
        batches = _tiny_batches(views)
        dec = BoxDecoder("Car", DEV, anchors=generate_anchors("Car")[:8, :12])
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        got = m.evaluate(batches, DEV, decoder=dec, decode=decode, tta=aug)
        assert m.training and all(mod.training for mod in m.modules())
        for k, v in m.state_dict().items():          # mode, parameters, running statistics: untouched
            assert torch.equal(v, state[k]), k
        # ---- the same pipeline from the public pieces
        want = DetectionEvaluator("Car", DEV)
        m.eval()
        hand, per_view_counts = [], []
        with torch.no_grad():
            for x in batches:
                pools = []
                for view in views:
                    if view.identity:
                        feats, coords = x[2], x[4]
                    else:
                        feats, coords = [], []
                        for b, raw in enumerate(x[6]):
                            pts = torch.from_numpy(np.ascontiguousarray(raw[:, :4])).to(DEV)
                            none = np.zeros((0, 7))
                            prm = A.ComposeParams(none, none, np.zeros(0, dtype=bool), np.zeros(0, dtype=A.MOVE_DTYPE), [], view.flip_y,
                                                  view.angle, view.scale, (0.0, 0.0, 0.0),
                                                  A.compose_affine(view.flip_y, view.angle, view.scale, None))
                            fb, cb, _ = voxelize_device(A.compose_points_device(pts, prm), g, b, coord_cols=4)
                            feats.append(fb)
                            coords.append(cb)
                    prob, delta = m.detect(feats, coords)
                    kw = dict(layout="site")
                    if heads:
                        from voxelnet_amd.anchor_mask import AnchorMasker
                        mask = AnchorMasker("Car", DEV, anchors=dec.anchors, threshold=1, grid=g).mask(_batch_cat(coords, torch.int64), 2)
                        kw.update(dir_logits=m.last_dir_logits, dir_offset=m.dir_offset, iou_logits=m.last_iou_logits,
                                  iou_rectify=m.iou_rectify, anchor_mask=mask)
                    pools.append(dec.candidates_device(prob, delta, 1e-6, 96, **kw))
                per_view_counts.append([p[3].tolist() for p in pools])
                mb, ms, src, mc = tta.merge_pools([p[0] for p in pools], [p[1] for p in pools], [p[3] for p in pools], views)
                keep, kc = nms_device(mb, mc, "rotated", 0.1, want.top_k)
                det = tta.vote_device(mb, ms, mc, keep, kc, vote, src=src, rows_per_view=96, n_views=3)[:3]
                want.update(*det, x[1])
                hand.append(det)
            # predict(tta=) on the first batch: the identity view's maps come from the caller
            m.__dict__["_decoder"] = dec
            prob, delta = m.detect(batches[0][2], batches[0][4])
            _, rows = m.predict(batches[0], prob, delta, decode=dict(decode, top_k=want.top_k), tta=aug)
        assert all(min(c) > 0 for cs in per_view_counts for c in cs), per_view_counts          # every view saw every frame
        _same_metrics(got.compute(), want.compute())
        assert got.compute()["n_det"] > 0
        hb, hs, hc = _host(*hand[0])
        for b in range(2):
            assert len(rows[b]) == hc[b]
            assert np.array_equal(rows[b][:, 1:8].astype(np.float32), hb[b, :hc[b]]) or \
                np.allclose(rows[b][:, 1:8].astype(np.float64), hb[b, :hc[b]], rtol=1e-6, atol=0)          # (via strings)
            assert np.allclose(rows[b][:, 8].astype(np.float64), hs[b, :hc[b]], rtol=1e-6, atol=0)
        with pytest.raises(Exception, match="eval"):
            m.train().predict(batches[0], prob, delta, decode=decode, tta=aug)
    finally:
        M.set_precision(before)
