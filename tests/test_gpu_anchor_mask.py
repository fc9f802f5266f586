"""GPU: the anchor mask (csrc/anchor_mask.hip, voxelnet_amd/anchor_mask.py, the anchor_mask argument
of targets.TargetGenerator / predict.BoxDecoder and RPN3D(anchor_area_threshold=)) against the NumPy restatement
tests/anchor_mask_ref.py on the inputs of tests/anchor_mask_cases.py, whose guards tests/test_anchor_mask_host.py asserts on
the reference alone.

Every quantity is an integer: mask, count, the edited pos / neg and the masked probs are compared for EXACT equality, floats
by their bits.  There is no tolerance anywhere in this file.

Grids (H, W) of the small cases, from the kernels' constants (AM_THREADS = the row scan's chunk, AM_SEG = rows per column
segment, read from the source by anchor_mask_cases): see anchor_mask_cases.GRIDS, which says which seam each one crosses —
(1, 1), (3, 5), (7, chunk), (7, chunk + 1), (seg, 9), (seg + 1, 9), (2 seg + 1, 9), (130, 300)."""
import numpy as np
import pytest
import torch

import anchor_mask_cases as C
import anchor_mask_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _mask_call(coord, B, H, W, rect, thr, pos=None, neg=None, fill=None, want_count=True):
    """vn_anchor_mask itself on NumPy inputs -> (mask (B,N) uint8, count (B,N) int32 or None) as NumPy arrays"""
    from voxelnet_amd import _lib
    N, K = rect.shape[0], coord.shape[0]
    nbytes = _lib.load().vn_anchor_mask_workspace_bytes(B, H, W, N)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    if fill is not None:
        ws.fill_(fill)
    c, r = (_dev(coord) if K else None), _dev(rect)
    mask = torch.full((B, N), 7, dtype=torch.uint8, device=DEV)
    count = torch.full((B, N), -7, dtype=torch.int32, device=DEV) if want_count else None
    _lib.call("vn_anchor_mask", c.data_ptr() if K else None, K, B, H, W, r.data_ptr(), N, thr, mask.data_ptr(),
              count.data_ptr() if want_count else None, None if pos is None else pos.data_ptr(), None if neg is None else neg.data_ptr(),
              ws.data_ptr(), nbytes, _lib.raw_stream())
    torch.cuda.synchronize()
    return mask.cpu().numpy(), (count.cpu().numpy() if want_count else None)


# ------------------------------------------------------------------------------------------------------ 1. small grids
@pytest.mark.parametrize("hw", list(C.GRIDS), ids=lambda s: "x".join(str(v) for v in s))
def test_small_grids_equal_brute_force(hw):
    """B = 3 with (many, 0, 1) voxels and four rows that must be ignored, hand-made rectangle tables, thresholds 0, 1, 5 and one
    above every count; then the same grid with K == 0.  Twice, the second time on a workspace of 0xFF bytes: bit-equal."""
    H, W = hw
    coord, rect = C.voxels(H, W), C.rect_table(H, W)
    ref = R.count_brute(coord, C.B, H, W, rect)
    assert ref[0].max() > 5 and ref[1].max() == 0 and ref[2].max() == 1
    for thr in C.THRESHOLDS + (int(ref.max()) + 1,):
        mask, count = _mask_call(coord, C.B, H, W, rect, thr)
        assert np.array_equal(count, ref), (hw, thr)
        assert np.array_equal(mask, R.mask_of(ref, thr)), (hw, thr)
        mask2, count2 = _mask_call(coord, C.B, H, W, rect, thr, fill=0xFF)
        assert np.array_equal(mask2, mask) and np.array_equal(count2, count), (hw, thr)
        mask3, none = _mask_call(coord, C.B, H, W, rect, thr, want_count=False)
        assert none is None and np.array_equal(mask3, mask)
    assert not R.mask_of(ref, int(ref.max()) + 1).any()
    mask, count = _mask_call(np.zeros((0, 4), dtype=np.int64), C.B, H, W, rect, 0, fill=0xFF)
    assert not mask.any() and not count.any()


# ------------------------------------------------------------------------------------------------------- 2. full grids
@pytest.mark.parametrize("cls_name", ["Car", "Pedestrian"])
def test_full_grids(cls_name):
    """the class's stock anchors on its full grid, B = 2, ~20 k seeded voxels per frame: equal to the cumsum reference
    everywhere and to brute force on 2,000 seeded anchors; two calls are bit-equal"""
    from voxelnet_amd.anchor_mask import AnchorMasker
    coord, g = C.full_frame(cls_name)
    mk = AnchorMasker(cls_name, DEV, threshold=1)
    mask, count = mk.mask(_dev(coord), 2, return_count=True)
    mask_again = mk.mask(_dev(coord), 2)
    h, w = mk.shape
    assert mask.shape == (2, h, w, 2) and mask.dtype == torch.uint8 and count.dtype == torch.int32
    ref = R.count_cumsum(coord, 2, g.H, g.W, mk.rects)
    assert np.array_equal(count.cpu().numpy().reshape(2, -1), ref)
    assert np.array_equal(mask.cpu().numpy().reshape(2, -1), R.mask_of(ref, 1)) and torch.equal(mask, mask_again)
    pick = np.random.default_rng(11).choice(mk.n_anchors, 2000, replace=False)
    assert np.array_equal(R.count_brute(coord, 2, g.H, g.W, mk.rects, pick), ref[:, pick])
    kept = R.mask_of(ref, 1).mean()
    print(f"{cls_name}: {coord.shape[0]} voxels, {kept:.3f} of {mk.n_anchors} anchors kept at threshold 1")
    assert 0.05 < kept < 0.95          # (the frame exercises both outcomes)


# ---------------------------------------------------------------------------------------------------- 3. in-place edit
def _sparse(counts, H, W, seed):
    rng = np.random.default_rng(seed)
    rows = [(b, int(rng.integers(0, C.D)), int(rng.integers(0, H)), int(rng.integers(0, W))) for b, k in enumerate(counts) for _ in range(k)]
    return np.array(rows, dtype=np.int64).reshape(-1, 4)


def _tiny_labels(anchors, picks):
    from voxelnet_amd.targets import lidar_box_to_label_line
    return [[lidar_box_to_label_line("Car", anchors[iy, ix, a]) for iy, ix, a in frame] for frame in picks]


def test_in_place_edit_of_fresh_targets():
    """pos / neg from TargetGenerator on frames with boxes: after the call they equal pos * mask, neg * mask bit for bit and
    targets is unchanged; a kept anchor's float NaN, planted by the test, survives: kept entries are not rewritten.  The
    generator's own anchor_mask= argument gives the same maps."""
    from test_gpu_dir_head import ANCHORS_TINY
    from voxelnet_amd.anchor_mask import AnchorMasker
    from voxelnet_amd.targets import TargetGenerator
    g = C.tiny_grid()
    labels = _tiny_labels(ANCHORS_TINY, [[(4, 6, 0)], [], [(2, 3, 1), (6, 9, 0)]])
    coord = _sparse((25, 8, 0), g.H, g.W, 3)
    for assign in ("reference", "rotated"):
        gen = TargetGenerator("Car", DEV, anchors=ANCHORS_TINY, assign=assign)
        mk = AnchorMasker("Car", DEV, anchors=ANCHORS_TINY, threshold=1, grid=g)
        ref = R.mask_of(R.count_brute(coord, 3, g.H, g.W, R.rects(ANCHORS_TINY, g)), 1)
        assert 0 < ref[0].sum() < ref[0].size and not ref[2].any()
        pos, neg, tgt = gen(labels)
        torch.cuda.synchronize()
        # (the reference's assignment, with its position-dependent union term, finds no positive on this slice of the grid)
        assert (float(pos.sum()) > 0) == (assign == "rotated") and float(neg.sum()) > 0
        plain = gen(labels, anchor_mask=mk.mask(_dev(coord), 3))
        p0, n0, t0 = _bits(pos).reshape(3, -1).copy(), _bits(neg).reshape(3, -1).copy(), _bits(tgt).copy()
        i = int(np.flatnonzero(ref.reshape(-1))[0])          # a kept anchor
        nan = np.float32(np.nan).view(np.int32)
        pos.view(-1)[i], neg.view(-1)[i] = float("nan"), float("nan")
        p0.reshape(-1)[i], n0.reshape(-1)[i] = nan, nan
        mask = mk.mask(_dev(coord), 3, pos=pos, neg=neg)
        torch.cuda.synchronize()
        assert np.array_equal(mask.cpu().numpy().reshape(3, -1), ref)
        assert np.array_equal(_bits(pos).reshape(3, -1), np.where(ref != 0, p0, 0)), assign
        assert np.array_equal(_bits(neg).reshape(3, -1), np.where(ref != 0, n0, 0)), assign
        assert np.array_equal(_bits(tgt), t0) and np.isnan(pos.view(-1)[i].item())
        p0.reshape(-1)[i], n0.reshape(-1)[i] = _bits(plain[0]).reshape(-1)[i], _bits(plain[1]).reshape(-1)[i]
        assert np.array_equal(_bits(plain[0]).reshape(3, -1), np.where(ref != 0, p0, 0))
        assert np.array_equal(_bits(plain[1]).reshape(3, -1), np.where(ref != 0, n0, 0)) and np.array_equal(_bits(plain[2]), t0)
        with pytest.raises(ValueError):
            gen(labels, anchor_mask=mask[:2])
        with pytest.raises(ValueError):
            mk.mask(_dev(coord), 3, pos=pos[:2], neg=neg[:2])


# ------------------------------------------------------------------------------------------------------------ 4. probs
@pytest.mark.parametrize("layout", ["flat", "site"])
def test_mask_probs(layout):
    """B = 2: kept entries bit-identical, masked entries exactly +0.0f, the input untouched"""
    from voxelnet_amd import _lib
    from voxelnet_amd.anchor_mask import AnchorMasker, mask_probs
    rng = np.random.default_rng(9)
    h, w = 5, 7
    probs = rng.random((2, 2, h, w)).astype(np.float32)
    probs[0, 0, 0, :3] = (-0.0, np.nan, np.inf)
    mask = (rng.random((2, h, w, 2)) < 0.5).astype(np.uint8)
    p = _dev(probs)
    out = mask_probs(p, _dev(mask), 2 * h * w, {"flat": _lib.VN_DETECT_FLAT, "site": _lib.VN_DETECT_SITE}[layout])
    torch.cuda.synchronize()
    assert np.array_equal(_bits(p), probs.view(np.int32))
    ref = R.masked_probs(probs, mask.reshape(2, -1), layout)
    assert np.array_equal(_bits(out), ref.view(np.int32)) and out.shape == p.shape
    zero = ref.view(np.int32) == 0
    assert zero.sum() >= (mask == 0).sum() and not np.signbit(out.cpu().numpy()[zero]).any()
    mk = AnchorMasker.__new__(AnchorMasker)
    mk.n_anchors = 2 * h * w
    assert torch.equal(mk.mask_probs(p, _dev(mask), layout).view(torch.int32), out.view(torch.int32))
    with pytest.raises(ValueError):
        mask_probs(p, _dev(mask)[:1], 2 * h * w, _lib.VN_DETECT_FLAT)
    with pytest.raises(_lib.VoxelnetHipError):
        _lib.call("vn_anchor_mask_probs", p.data_ptr(), _dev(mask).data_ptr(), 2, 2 * h * w, _lib.VN_DETECT_FLAT, p.data_ptr(), None)


# ------------------------------------------------------------------------------------------------------------ 5. model
TINY_PICKS = [[(4, 6, 0), (1, 2, 1)], [(6, 3, 0)]]


def _labelled(golden):
    from test_gpu_dir_head import ANCHORS_TINY, _tiny
    _, coords, _, batch = _tiny(golden)
    labels = _tiny_labels(ANCHORS_TINY, TINY_PICKS)
    return (batch[0], labels) + batch[2:], torch.cat(coords).numpy()


def _public_targets(threshold, assign="reference", keep_heading=False):
    """what a caller builds from the public pieces: TargetGenerator + AnchorMasker"""
    from test_gpu_dir_head import ANCHORS_TINY
    from voxelnet_amd.anchor_mask import AnchorMasker
    from voxelnet_amd.targets import TargetGenerator
    gen = TargetGenerator("Car", DEV, anchors=ANCHORS_TINY, assign=assign, keep_heading=keep_heading)
    return gen, AnchorMasker("Car", DEV, anchors=ANCHORS_TINY, threshold=threshold, grid=C.tiny_grid())


def _same(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.isfinite(x).all() and torch.equal(_dev_bits(x), _dev_bits(y)), (what, i)


def _dev_bits(t):
    return t.detach().float().contiguous().view(torch.int32)


@pytest.mark.parametrize("thr", [1, 20])
@pytest.mark.parametrize("dir_head", [False, True], ids=["native", "dir_head"])
@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_model_masks_its_own_targets(golden, monkeypatch, mode, dir_head, thr):
    """The tiny golden batch at threshold 1 — where every one of its 2 x 192 anchors has at least 10 voxels under it, so the
    reference masks nothing out and the model must equal the default model bit for bit — and at threshold 20, where the
    reference masks out 12 + 3 anchors.  forward == forward(targets=...) with targets built from the public pieces, bit
    for bit (maps and five scalars); train_step == forward + backward bit for bit (maps, scalars, every gradient) — through
    the fused call (vn_net_step) without the direction head, on the per-layer path with it; the negatives the model's loss
    sees are fewer than the unmasked ones by exactly the number of negatives the reference masks out (0 at threshold 1), and
    cneg differs exactly when that number is not 0.  Targets: the reference's assignment for the default configuration
    (native executor, threshold 1; on this slice of the grid it finds no positive), assignment by the rotated IoU — with
    positives — everywhere else."""
    from test_gpu_dir_head import ANCHORS_TINY, _tiny_model
    from voxelnet_amd.targets import TargetGenerator
    assign = "reference" if thr == 1 and not dir_head else "rotated"

    def model(**extra):
        m = _tiny_model(mode, target_assign=assign, **kw, **extra)
        m.__dict__["_targets"] = TargetGenerator("Car", DEV, anchors=ANCHORS_TINY, assign=assign, keep_heading=dir_head)
        return m
    from voxelnet_amd import _lib
    from voxelnet_amd import model as M
    batch, coord = _labelled(golden)
    g = C.tiny_grid()
    ref = R.mask_of(R.count_brute(coord, 2, g.H, g.W, R.rects(ANCHORS_TINY, g)), thr)
    assert (ref == 0).sum(axis=1).tolist() == {1: [0, 0], 20: [12, 3]}[thr]
    kw = dict(dir_head=True) if dir_head else {}
    names, real = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    try:
        a = model(anchor_area_threshold=thr)
        out_a = a(batch, DEV)
        out_a[2].backward()
        assert np.array_equal(a.last_anchor_mask.cpu().numpy().reshape(2, -1), ref) and not a.last_anchor_mask.requires_grad
        gen, mk = _public_targets(thr, assign=assign, keep_heading=dir_head)
        pos, neg, tgt = gen(batch[1])
        assert (float(pos.sum()) > 0) == (assign == "rotated")
        neg_before = neg.clone()
        mk.mask(torch.cat(batch[4]), 2, pos=pos, neg=neg)
        b = model(anchor_area_threshold=thr)
        out_b = b(batch, DEV, targets=(pos, neg, tgt))
        _same(out_a, out_b, "forward vs forward(targets=)")
        c = model(anchor_area_threshold=thr)
        assert c._step_fused_ok(mode, None) == (not dir_head)
        monkeypatch.setattr(_lib, "call", recording)
        out_c = c.train_step(batch, DEV, None)
        monkeypatch.setattr(_lib, "call", real)
        assert ("vn_net_step" in names) == (not dir_head) and "vn_anchor_mask" in names
        d = model()
        out_d = d(batch, DEV)
        torch.cuda.synchronize()
    finally:
        monkeypatch.setattr(_lib, "call", real)
        M.set_precision("bf16")
    _same(out_a, out_c, "train_step vs forward + backward")
    ga, gc = dict(a.named_parameters()), dict(c.named_parameters())
    assert len(ga) == (106 if dir_head else 104)
    for k in ga:
        assert ga[k].grad is not None and torch.isfinite(ga[k].grad).all() and torch.equal(_dev_bits(ga[k].grad), _dev_bits(gc[k].grad)), k
    assert np.array_equal(c.last_anchor_mask.cpu().numpy().reshape(2, -1), ref) and d.last_anchor_mask is None
    nb = neg_before.cpu().numpy().reshape(2, -1)
    dropped = int(((nb != 0) & (ref == 0)).sum())
    assert (dropped > 0) == (thr == 20) and int(nb.sum()) - int(neg.sum().item()) == dropped
    assert (float(out_a[6].detach()) != float(out_d[6].detach())) == (dropped > 0)
    if thr == 1:
        _same(out_a, out_d, "nothing masked out: the default model")
    print(f"{mode} dir_head={dir_head} {assign}: {int(ref.sum())} of {ref.size} anchors kept, {dropped} negatives ignored, "
          f"cneg {float(out_d[6].detach()):.6f} -> {float(out_a[6].detach()):.6f}")


# ------------------------------------------------------------------------------------------------------- 6. round trip
CAR, GHOST = (7, 6, 0), (0, 3, 0)          # (iy, ix, a) on the 8 x 12 slice of the anchor grid


def _round_trip(layout):
    """one car with voxels under it and a ghost — an anchor over cells without a voxel —, both scoring 0.9, every other
    anchor 0.05; deltas zero (a detection is its anchor)"""
    from test_gpu_dir_head import ANCHORS_TINY
    g = C.tiny_grid()
    coord = np.array([(0, d, h, w) for d, h, w in [(1, 11, 10), (2, 11, 13), (1, 12, 12), (3, 12, 15), (1, 13, 16), (2, 13, 11)]], dtype=np.int64)
    n_car, n_ghost = ((iy * 12 + ix) * 2 + a for iy, ix, a in (CAR, GHOST))
    cnt = R.count_brute(coord, 1, g.H, g.W, R.rects(ANCHORS_TINY, g))
    assert cnt[0, n_car] == 6 and cnt[0, n_ghost] == 0          # the guard, on the reference
    probs = np.full((1, 2, 8, 12), 0.05, dtype=np.float32)
    for iy, ix, a in (CAR, GHOST):
        if layout == "site":
            probs[0, a, iy, ix] = 0.9
        else:
            probs.reshape(-1)[(iy * 12 + ix) * 2 + a] = 0.9
    return coord, _dev(probs), torch.zeros((1, 14, 8, 12), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("layout", ["flat", "site"])
def test_round_trip_ghost_in_empty_space(layout):
    """The test that fails without the feature.  With the mask decode_device returns exactly one detection, the car's;
    without it two — the ghost over empty cells passes score_thres —; the car's box and score are bit-identical in both."""
    from test_gpu_dir_head import ANCHORS_TINY
    from voxelnet_amd.anchor_mask import AnchorMasker
    from voxelnet_amd.predict import BoxDecoder
    coord, probs, deltas = _round_trip(layout)
    dec = BoxDecoder("Car", DEV, anchors=ANCHORS_TINY, layout=layout)
    mk = AnchorMasker("Car", DEV, anchors=ANCHORS_TINY, threshold=1, grid=C.tiny_grid())
    mask = mk.mask(_dev(coord), 1)
    kw = dict(score_thres=0.5, nms="rotated", pre_nms_top_k=64, top_k=20)
    without = dec.decode_device(probs, deltas, **kw)
    with_mask = dec.decode_device(probs, deltas, **kw, anchor_mask=mask)
    assert without[2].tolist() == [2] and with_mask[2].tolist() == [1]
    car = ANCHORS_TINY[CAR]
    rows = without[0][0, :2].cpu().numpy()
    j = int(np.argmin(np.abs(rows[:, 1] - car[1])))
    assert np.allclose(rows[j, :2], car[:2], atol=1e-5) and np.allclose(with_mask[0][0, 0, :2].cpu().numpy(), car[:2], atol=1e-5)
    assert torch.equal(_dev_bits(with_mask[0][0, 0]), _dev_bits(without[0][0, j]))
    assert torch.equal(_dev_bits(with_mask[1][0, 0]), _dev_bits(without[1][0, j]))
    cand = dec.candidates_device(probs, deltas, 0.5, 64, anchor_mask=mask)
    assert cand[3].tolist() == [1] and dec.candidates_device(probs, deltas, 0.5, 64)[3].tolist() == [2]
    boxes, scores = dec(probs, deltas, **kw, anchor_mask=mask)
    assert len(boxes) == 1 and boxes[0].shape == (1, 7) and scores[0].shape == (1,)
    with pytest.raises(ValueError, match="score_thres"):
        dec.decode_device(probs, deltas, **dict(kw, score_thres=0.0), anchor_mask=mask)
    with pytest.raises(ValueError):
        dec.decode_device(probs, deltas, **kw, anchor_mask=torch.ones((2, 8, 12, 2), dtype=torch.uint8, device=DEV))


def test_round_trip_through_the_model(golden, monkeypatch):
    """the same frame through RPN3D.evaluate / predict: anchor_area_threshold=1 leaves one detection, the default two"""
    from test_gpu_dir_head import ANCHORS_TINY, _tiny_model
    from voxelnet_amd import model as M
    from voxelnet_amd.evaluate import DetectionEvaluator
    from voxelnet_amd.predict import TRAINED_DECODE, BoxDecoder
    coord, probs, deltas = _round_trip("site")
    labels = _tiny_labels(ANCHORS_TINY, [[CAR]])
    feats = [torch.zeros((coord.shape[0], 35, 7), dtype=torch.float32, device=DEV)]
    batch = (["000000"], labels, feats, None, [_dev(coord)], None, None)
    decode = dict(TRAINED_DECODE, score_thres=0.5)
    try:
        n_det = {}
        for name, kw in (("mask", dict(anchor_area_threshold=1)), ("default", {})):
            m = _tiny_model("bf16", **kw)
            monkeypatch.setattr(m, "detect", lambda f, c: (probs, deltas))
            dec = BoxDecoder("Car", DEV, anchors=ANCHORS_TINY)
            ev = m.evaluate([batch], DEV, evaluator=DetectionEvaluator("Car", DEV), decoder=dec, decode=decode)
            n_det[name] = ev.compute()["n_det"]
            m.__dict__["_decoder"] = dec
            _, rows = m.predict(batch, probs, deltas, decode=dict(decode, top_k=20))
            assert len(rows) == 1 and len(rows[0]) == n_det[name]
            assert (m.last_anchor_mask is not None) == (name == "mask")
            if name == "mask":
                with pytest.raises(ValueError, match="score_thres"):
                    m.predict(batch, probs, deltas, decode=dict(decode, score_thres=0.0))
                with pytest.raises(Exception, match="coordinates"):
                    m.predict((batch[0],), probs, deltas, decode=decode)
        assert n_det == {"mask": 1, "default": 2}
    finally:
        M.set_precision("bf16")
