"""GPU: detection scoring (csrc/eval.hip through vn_box_iou_rotated / vn_eval_match, voxelnet_amd/evaluate.py,
BoxDecoder.decode_device, RPN3D.evaluate) against the float64 restatement tests/eval_ref.py.

Bars.  Pairwise IoU: |device - reference| <= 1e-9 — both sides are float64 on coordinates <= 100 m, the reference's own
operand-order spread is below 1e-15, so 1e-9 leaves six orders for another operation order and still sits four orders
under the threshold margin the matching tests require of their inputs.  Matching: the test first asserts ON THE REFERENCE
ALONE that no IoU of its inputs lies within 1e-6 of the threshold (a condition on the inputs: nothing is left out of the
comparison); then status and matched_gt must equal the reference exactly.  AP: 1e-12 (with identical statuses it is the
same rational arithmetic)."""
import functools
import math

import numpy as np
import pytest
import torch

import eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IOU_TOL = 1e-9
MARGIN = 1e-6
TOP_K = 20


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------ inputs
def _grid_gts(n=128):
    """n disjoint car-sized ground truths on a 13 x 10 grid, headings alternating"""
    out = []
    for k in range(n):
        i, j = k % 13, k // 13
        out.append([6.0 + 5.0 * i, -31.5 + 7.0 * j, -1.6, 1.5, 1.6, 4.0, 0.3 * ((k % 5) - 2)])
    return np.array(out, dtype=np.float64)


def _jitter(rng, g):
    d = np.array(g, dtype=np.float64)
    d[0:2] += rng.normal(0, 0.15, 2)
    d[2] += rng.normal(0, 0.05)
    d[6] += rng.normal(0, 0.05)
    d[3:6] *= rng.uniform(0.95, 1.05, 3)
    return d


def _frame(det, scores, gt, flags):
    det = np.asarray(det, dtype=np.float64).reshape(-1, 7).astype(np.float32)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 7)
    flags = np.asarray(flags, dtype=bool).reshape(len(R.DIFFS), gt.shape[0])
    return {"det": det, "scores": np.asarray(scores, dtype=np.float32), "gt": gt, "flags": flags}


def _hand_frames():
    rng = np.random.default_rng(77)
    car = [20.0, 3.0, -1.6, 1.5, 1.6, 4.0, 0.2]
    three = np.array([car, [30.0, -8.0, -1.6, 1.5, 1.6, 4.0, -1.0], [44.0, 12.0, -1.5, 1.6, 1.7, 4.2, 1.3]])
    none4 = np.zeros((4, 0), dtype=bool)
    frames = []
    # no detections
    frames.append(_frame(np.zeros((0, 7)), [], three, np.zeros((4, 3), dtype=bool)))
    # no ground truths
    frames.append(_frame([_jitter(rng, g) for g in three], [0.99, 0.98, 0.97], np.zeros((0, 7)), none4))
    # 128 ground truths (both ground-truth slots of a lane in use), every third one ignored at the last two difficulties
    grid = _grid_gts(128)
    fl = np.zeros((4, 128), dtype=bool)
    fl[2:, ::3] = True
    fl[1, 64:] = True
    picks = [0, 3, 5, 63, 64, 65, 66, 90, 99, 100, 126, 127, 12, 13, 14, 77, 78, 81]
    det = [_jitter(rng, grid[k]) for k in picks] + [[40.0, 38.0, -1.6, 1.5, 1.6, 4.0, 0.0], _jitter(rng, grid[127])]
    frames.append(_frame(det, 0.96 + 0.001 * rng.permutation(20), grid, fl))
    # 20 detections on one ground truth: one takes it, the others are false positives
    frames.append(_frame([_jitter(rng, car) for _ in range(20)], 0.96 + 0.0015 * rng.permutation(20), [car],
                         [[False], [False], [True], [False]]))
    # two detections with EQUAL scores on one ground truth: the lower index walks first and takes it, although the
    # second overlaps more
    worse = list(car)
    worse[0] += 0.25
    frames.append(_frame([worse, car, _jitter(rng, three[1])], [0.98, 0.98, 0.98], three, np.zeros((4, 3), dtype=bool)))
    # one detection overlapping two ground truths EQUALLY (mirror images in y, dyadic numbers: every operation is exact or
    # mirrored): the lower index is taken; where that one is ignored and the other valid, the valid one
    det = [[16.0, 0.0, -1.5, 1.5, 4.0, 4.0, 0.0]]
    pair = [[16.0, 0.25, -1.5, 1.5, 4.0, 4.0, 0.0], [16.0, -0.25, -1.5, 1.5, 4.0, 4.0, 0.0]]
    frames.append(_frame(det, [0.97], pair, [[False, False], [True, False], [True, True], [False, True]]))
    return frames


@functools.lru_cache(maxsize=None)
def _case(name):
    """the frames of a case with the reference's IoU tables, computed once and shared (never modified)"""
    if name == "hand":
        frames = _hand_frames()
    else:
        frames = []
        for det, scores, lines in R.make_scene(int(name)):
            gt, flags = R.frame_ground_truth(lines)
            f = _frame(det, scores, gt, flags)
            f["lines"] = lines
            frames.append(f)
    for f in frames:
        det = f["det"].astype(np.float64)
        iou = np.zeros((2, det.shape[0], f["gt"].shape[0]), dtype=np.float64)
        for i in range(det.shape[0]):
            for j in range(f["gt"].shape[0]):
                iou[:, i, j] = R.iou_pair(det[i], f["gt"][j])
        iou.setflags(write=False)
        f["iou"] = iou
    return frames


def _run_match(frames, thr_bev, thr_3d, top_k=TOP_K, want_iou=True):
    """vn_eval_match on the frames as ONE batch -> status, matched, iou_out (or None), walk order: host arrays"""
    from voxelnet_amd import _lib
    B = len(frames)
    G = max([f["gt"].shape[0] for f in frames] + [1])
    n_diff = len(R.DIFFS)
    det = np.zeros((B, top_k, 7), dtype=np.float32)
    sc = np.zeros((B, top_k), dtype=np.float32)
    dc = np.zeros(B, dtype=np.int32)
    gt = np.zeros((B, G, 7), dtype=np.float64)
    gc = np.zeros(B, dtype=np.int32)
    fl = np.zeros((B, n_diff, G), dtype=np.uint8)
    for b, f in enumerate(frames):
        n, g = f["det"].shape[0], f["gt"].shape[0]
        det[b, :n], sc[b, :n], dc[b] = f["det"], f["scores"], n
        gt[b, :g], gc[b] = f["gt"], g
        fl[b, :, :g] = f["flags"]
    det_d, sc_d, dc_d, gt_d, gc_d, fl_d = (_dev(a) for a in (det, sc, dc, gt, gc, fl))
    status = torch.full((B, 2, n_diff, top_k), 99, dtype=torch.int8, device=DEV)
    matched = torch.full((B, 2, n_diff, top_k), -99, dtype=torch.int32, device=DEV)
    iou = torch.full((B, 2, top_k, G), -1.0, dtype=torch.float64, device=DEV) if want_iou else None
    nbytes = _lib.load().vn_eval_match_workspace_bytes(B, top_k, G)
    assert nbytes >= B * top_k * 4
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    _lib.call("vn_eval_match", det_d.data_ptr(), sc_d.data_ptr(), dc_d.data_ptr(), gt_d.data_ptr(), gc_d.data_ptr(), fl_d.data_ptr(),
              B, top_k, G, n_diff, float(thr_bev), float(thr_3d), status.data_ptr(), matched.data_ptr(),
              iou.data_ptr() if want_iou else None, ws.data_ptr(), nbytes, _lib.raw_stream())
    torch.cuda.synchronize()
    order = ws.cpu().numpy()[:B * top_k * 4].view(np.int32).reshape(B, top_k)
    return status.cpu().numpy(), matched.cpu().numpy(), iou.cpu().numpy() if want_iou else None, order


def _reference_match(frames, thr_bev, thr_3d, top_k=TOP_K):
    B, n_diff = len(frames), len(R.DIFFS)
    status = np.full((B, 2, n_diff, top_k), -2, dtype=np.int64)
    matched = np.full((B, 2, n_diff, top_k), -1, dtype=np.int64)
    order = np.full((B, top_k), -1, dtype=np.int64)
    for b, f in enumerate(frames):
        n = f["det"].shape[0]
        order[b, :n] = sorted(range(n), key=lambda d: (-float(f["scores"][d]), d))
        for m, thr in enumerate((thr_bev, thr_3d)):
            for k in range(n_diff):
                status[b, m, k, :n], matched[b, m, k, :n] = R.match_frame(f["iou"][m], f["scores"], f["flags"][k], thr)
    return status, matched, order


def _assert_margin(frames, thrs):
    """the precondition, on the reference alone: no IoU within MARGIN of a threshold in use"""
    closest = min((abs(float(v) - t) for f in frames for v in f["iou"].reshape(-1) for t in thrs), default=1.0)
    assert closest > MARGIN, f"an input IoU lies {closest:.2e} from its threshold: choose other inputs"
    return closest


# ------------------------------------------------------------------------------------------------ pairwise IoU
def _closed_form_boxes():
    x, y, z, h, w, l, r = 20.0, -3.0, -1.5, 1.6, 1.7, 4.2, 0.4
    return np.array([
        [x, y, z, h, w, l, r],
        [x, y, z, h, l, w, r + math.pi / 2],                                     # the twin: IoU 1
        [x + l / 2 * math.cos(r), y + l / 2 * math.sin(r), z, h, w, l, r],       # shifted by l/2 along the heading: 1/3
        [x, y, z + h / 2, h, w, l, r],                                           # half vertical overlap: 3D 1/3
        [x + 0.1, y + 0.1, z + 0.2, 1.0, 0.5, 1.2, -0.9],                       # contained
        [x + 50, y, z, h, w, l, r],                                              # disjoint
        [10.0, 2.0, -1.0, 1.5, 2.0, 4.0, 0.0], [14.0, 2.0, -1.0, 1.5, 2.0, 4.0, 0.0],          # touching along x = 12
        [12.0, 2.5, -1.78, 1.56, 1.6, 3.9, 0.0], [12.4, 2.9, -1.78, 1.56, 1.6, 3.9, math.pi / 2],   # the anchors' headings
        [11.0, 2.0, -1.0, 1.5, 0.0, 4.0, 0.0],                                   # zero width
        [11.0, 2.0, -1.0, 1.5, 2.0, 4.0, float("nan")], [float("inf"), 2.0, -1.0, 1.5, 2.0, 4.0, 0.0],
        [11.0, 2.0, -1.0, -1.5, 2.0, 4.0, 0.0],
    ], dtype=np.float64)


def _iou_inputs(shape):
    frames = _case("0")
    dets = np.concatenate([f["det"] for f in frames]).astype(np.float64)
    if shape == (1, 1):
        return dets[:1], dets[:1].copy()
    if shape == (20, 13):          # one crowded frame's detections and ground truths, filled up from its neighbours
        k = max(range(len(frames)), key=lambda i: frames[i]["det"].shape[0] * frames[i]["gt"].shape[0])
        a = np.concatenate([frames[k]["det"].astype(np.float64), dets])[:20]
        b = np.concatenate([frames[k]["gt"]] + [f["gt"] for f in frames])[:13]
        return a, b
    if shape == (3, 128):
        grid = _grid_gts(128)
        rng = np.random.default_rng(3)
        return np.array([_jitter(rng, grid[k]) for k in (0, 64, 127)]), grid
    if shape == (0, 5):
        return np.zeros((0, 7)), dets[:5]
    boxes = _closed_form_boxes()
    return boxes, boxes.copy()


@pytest.mark.parametrize("metric", ["bev", "3d"])
@pytest.mark.parametrize("shape", [(1, 1), (20, 13), (3, 128), (0, 5), "closed forms"])
def test_box_iou_rotated_vs_reference(shape, metric):
    from voxelnet_amd.evaluate import box_iou_rotated
    a, b = _iou_inputs(shape)
    got = box_iou_rotated(_dev(a), _dev(b), metric)
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (a.shape[0], b.shape[0])
    got = got.cpu().numpy()
    ref = R.iou_matrix(a, b, metric)
    assert np.isfinite(got).all()
    diff = float(np.abs(got - ref).max()) if got.size else 0.0
    print(f"box_iou_rotated {shape} {metric}: {got.size} pairs, {int((ref > 0).sum())} overlapping, max |device - reference| = {diff:.3e}")
    assert diff <= IOU_TOL
    if shape == (1, 1):
        assert abs(got[0, 0] - 1) <= IOU_TOL
    if shape == "closed forms":
        k = 0 if metric == "bev" else 1
        want = {(0, 0): 1.0, (0, 1): 1.0, (0, 2): 1 / 3, (0, 3): (1.0, 1 / 3)[k], (0, 5): 0.0, (6, 7): 0.0,
                (0, 4): ((0.5 * 1.2) / (1.7 * 4.2), (1.0 * 0.5 * 1.2) / (1.6 * 1.7 * 4.2))[k]}
        for (i, j), v in want.items():
            assert abs(got[i, j] - v) <= IOU_TOL and abs(got[j, i] - v) <= IOU_TOL, (i, j)
        assert (got[10:] == 0).all() and (got[:, 10:] == 0).all()          # degenerate boxes: 0, never NaN
    if shape == (20, 13):
        assert (ref > 0.5).sum() >= 5          # (the case does compare overlapping pairs)


def test_box_iou_rotated_widens_float32_exactly():
    from voxelnet_amd.evaluate import box_iou_rotated
    a, b = _iou_inputs((20, 13))
    a32 = a.astype(np.float32)
    got = box_iou_rotated(_dev(a32), _dev(b), "3d").cpu().numpy()
    assert float(np.abs(got - R.iou_matrix(a32.astype(np.float64), b, "3d")).max()) <= IOU_TOL


# ---------------------------------------------------------------------------------------------------- matching
@pytest.mark.parametrize("thr", [0.7, 0.5, 0.25])
@pytest.mark.parametrize("case", ["0", "1", "2", "3", "hand"])
def test_match_vs_reference(case, thr):
    frames = _case(case)
    closest = _assert_margin(frames, (thr,))
    status, matched, iou, order = _run_match(frames, thr, thr)
    ref_status, ref_matched, ref_order = _reference_match(frames, thr, thr)
    worst = 0.0
    for b, f in enumerate(frames):
        n, g = f["det"].shape[0], f["gt"].shape[0]
        if n and g:
            worst = max(worst, float(np.abs(iou[b, :, :n, :g] - f["iou"]).max()))
        pad = iou[b].copy()
        pad[:, :n, :g] = 0
        assert (pad == 0).all(), b          # beyond the counts: 0
    print(f"match {case} thr {thr}: {len(frames)} frames, closest IoU to the threshold {closest:.2e}, "
          f"max |iou_out - reference| = {worst:.3e}, TP/FP/ignored = "
          f"{int((ref_status == 1).sum())}/{int((ref_status == 0).sum())}/{int((ref_status == -1).sum())}")
    assert worst <= IOU_TOL
    assert np.array_equal(order, ref_order)
    assert np.array_equal(status, ref_status)
    assert np.array_equal(matched, ref_matched)
    # without the IoU tables asked for: the same statuses
    status2, matched2, _, _ = _run_match(frames, thr, thr, want_iou=False)
    assert np.array_equal(status2, status) and np.array_equal(matched2, matched)


def test_match_hand_frames_do_what_they_were_built_for():
    """the reference's own answers on the hand-made frames are the ones the frames were built to provoke (so the
    comparison above covers them): ties, exhaustion, ignored-after-valid"""
    frames = _case("hand")
    st, mg, _ = _reference_match(frames, 0.7, 0.7)
    assert (st[0] == -2).all() and (st[1][:, :, :3] == 0).all()
    assert ((st[3][:, :, :20] != 0).sum(axis=-1) == 1).all()                      # 20 on one: one match per matching
    assert (st[3][:, 2, :20] == -1).sum() == 2 and (st[3][:, 0, :20] == 1).sum() == 2
    assert (st[4][0, :, 0] == 1).all() and (st[4][0, :, 1] == 0).all()            # equal scores: index 0 first
    assert mg[5][0, :, 0].tolist() == [0, 1, 0, 0] and st[5][0, :, 0].tolist() == [1, 1, -1, 1]
    assert len(set(frames[5]["iou"][0].reshape(-1).tolist())) == 1                # exactly equal overlaps
    assert (mg[2] >= 64).any() and (st[2] == -1).any()


def test_match_two_thresholds_and_the_size_limits():
    """thr_bev != thr_3d reach their own metric; top_k = 32 with 128 ground truths is the largest launch (64 KB of LDS)"""
    grid = _grid_gts(128)
    rng = np.random.default_rng(9)
    det = [_jitter(rng, grid[k]) for k in range(0, 128, 4)]
    f = _frame(det, 0.96 + 0.001 * rng.permutation(32), grid, np.zeros((4, 128), dtype=bool))
    det64 = f["det"].astype(np.float64)
    f["iou"] = np.stack([R.iou_matrix(det64, grid, m) for m in ("bev", "3d")])
    frames = [f, _case("hand")[4]]
    _assert_margin(frames, (0.7, 0.5))
    status, matched, iou, order = _run_match(frames, 0.7, 0.5, top_k=32)
    ref_status, ref_matched, ref_order = _reference_match(frames, 0.7, 0.5, top_k=32)
    assert np.array_equal(status, ref_status) and np.array_equal(matched, ref_matched) and np.array_equal(order, ref_order)
    assert float(np.abs(iou[0] - f["iou"]).max()) <= IOU_TOL
    assert (ref_status[0, 0] != ref_status[0, 1]).any()          # (the two thresholds do decide differently here)


# ------------------------------------------------------------------------------------------------ AP end to end
@functools.lru_cache(maxsize=None)
def _ap_scene():
    """seed 0's 64 frames + 3 frames with a Van (ignored everywhere) that a detection sits on and a Pedestrian (dropped);
    the reference fed frame by frame"""
    scene = list(R.make_scene(0))
    rng = np.random.default_rng(123)
    for det, scores, lines in R.make_scene(100, n_frames=3):
        van = [rng.uniform(10, 60), rng.uniform(-30, 30), -1.7, 2.1, 1.9, 5.0, rng.uniform(-1.5, 1.5)]
        lines = lines + [R.label_line("Van", van), R.label_line("Pedestrian", [12.0, 3.0, -1.5, 1.7, 0.6, 0.8, 0.3])]
        det = np.concatenate([det[:19], np.array([van], dtype=np.float32)])
        scores = np.concatenate([scores[:19], np.array([0.9999], dtype=np.float32)])
        scene.append((det, scores, lines))
    ref = R.RefEvaluator("Car")
    ignored = 0
    for det, scores, lines in scene:
        ignored += int((ref.add_frame(det, scores, lines)["status"]["bev"][0] == -1).sum())
    assert ignored >= 3
    return scene, ref.compute()


def _feed(ev, scene, batch, device_form):
    for i in range(0, len(scene), batch):
        part = scene[i:i + batch]
        labels = [p[2] for p in part]
        if device_form:
            B = len(part)
            boxes, scores, counts = np.zeros((B, TOP_K, 7), np.float32), np.zeros((B, TOP_K), np.float32), np.zeros(B, np.int32)
            for b, (d, s, _) in enumerate(part):
                boxes[b, :len(s)], scores[b, :len(s)], counts[b] = d, s, len(s)
            ev.update(_dev(boxes), _dev(scores), _dev(counts), labels)
        else:
            ev.update([p[0] for p in part], [p[1] for p in part], None, labels)


def _assert_same_result(got, ref):
    assert set(got) == {"bev", "3d", "n_gt", "n_det"}
    assert got["n_det"] == ref["n_det"] and got["n_gt"] == ref["n_gt"]
    for m in ("bev", "3d"):
        assert list(got[m]) == list(R.DIFFS)
        for d in R.DIFFS:
            assert abs(got[m][d] - ref[m][d]) <= 1e-12, (m, d, got[m][d], ref[m][d])


@pytest.mark.parametrize("batch,device_form", [(2, True), (7, True), (7, False), (2, False)])
def test_average_precision_end_to_end(batch, device_form):
    from voxelnet_amd.evaluate import DetectionEvaluator
    scene, ref = _ap_scene()
    assert len(scene) % 7 != 0          # (a ragged last batch)
    ev = DetectionEvaluator("Car", DEV)
    _feed(ev, scene, batch, device_form)
    got = ev.compute()
    print(f"AP batch {batch} {'device' if device_form else 'list'} form: " + ", ".join(
        f"{m}/{d} {got[m][d]:.6f}" for m in ("bev", "3d") for d in R.DIFFS) + f"; n_gt {got['n_gt']}, n_det {got['n_det']}")
    _assert_same_result(got, ref)
    assert all(0 < got[m][d] < 1 for m in ("bev", "3d") for d in R.DIFFS)
    _assert_same_result(ev.compute(), ref)          # compute() twice
    ev.reset()
    assert ev.compute()["n_det"] == 0 and math.isnan(ev.compute()["bev"]["all"])
    _feed(ev, scene, batch, device_form)
    _assert_same_result(ev.compute(), ref)


def test_average_precision_r11_and_other_thresholds():
    from voxelnet_amd.evaluate import DetectionEvaluator
    scene = _ap_scene()[0][:16]
    ref = R.RefEvaluator("Car", diffs=("hard", "all"), thr=0.5, recall_points=11)
    for det, scores, lines in scene:
        ref.add_frame(det, scores, lines)
    ev = DetectionEvaluator("Car", DEV, iou_thres=0.5, difficulties=("hard", "all"), recall_points=11)
    _feed(ev, scene, 5, True)
    got, want = ev.compute(), ref.compute()
    assert got["n_gt"] == want["n_gt"] and got["n_det"] == want["n_det"]
    for m in ("bev", "3d"):
        for d in ("hard", "all"):
            assert abs(got[m][d] - want[m][d]) <= 1e-12


@functools.lru_cache(maxsize=None)
def _class_scene(cls):
    """16 frames of the class (its ranges, box sizes, anchor-sized false positives) with label lines of OTHER classes
    mixed in on top of detections and ground truths -> (scene, the reference's result, the reference's result with the
    other classes' lines taken out, per-frame IoU tables).  The reference is tests/eval_ref.py with the class's 0.5."""
    scene = R.make_scene(1, n_frames=16, cls_name=cls, others=True)
    ref, own = R.RefEvaluator(cls), R.RefEvaluator(cls)
    frames, n_other = [], 0
    for det, scores, lines in scene:
        r = ref.add_frame(det, scores, lines)
        mine = [l for l in lines if l.split()[0] == cls]
        n_other += len(lines) - len(mine)
        own.add_frame(det, scores, mine)
        frames.append({"iou": np.stack([r["iou"]["bev"], r["iou"]["3d"]])})
    assert n_other >= 16
    return scene, ref.compute(), own.compute(), frames


@pytest.mark.parametrize("batch", [2, 7])
@pytest.mark.parametrize("cls", ["Pedestrian", "Cyclist"])
def test_average_precision_other_classes(cls, batch):
    """DetectionEvaluator(cls) with its default threshold (IOU_THRES: 0.5) against RefEvaluator(cls); the Car, Van,
    Person_sitting, DontCare, ... lines in the labels are dropped: the result is the one without them"""
    from voxelnet_amd.evaluate import IOU_THRES, DetectionEvaluator
    scene, ref, ref_own, frames = _class_scene(cls)
    assert IOU_THRES[cls] == R.THRES[cls] == 0.5 and len(scene) == 16
    closest = _assert_margin(frames, (0.5,))
    ev = DetectionEvaluator(cls, DEV)
    assert ev.iou_thres == (0.5, 0.5)
    _feed(ev, scene, batch, True)
    got = ev.compute()
    print(f"AP {cls} batch {batch}: closest IoU to 0.5 {closest:.2e}; " + ", ".join(
        f"{m}/{d} {got[m][d]:.6f}" for m in ("bev", "3d") for d in R.DIFFS) + f"; n_gt {got['n_gt']}, n_det {got['n_det']}")
    _assert_same_result(got, ref)
    _assert_same_result(got, ref_own)
    assert all(0 < got[m][d] < 1 for m in ("bev", "3d") for d in R.DIFFS)


# ------------------------------------------------------------------------------- decode_device, RPN3D.evaluate
@pytest.mark.parametrize("which", ["fixture maps", (5, False), (6, True)])
def test_decode_device_is_call_without_the_copies(which):
    from oracle import targets as ot
    from voxelnet_amd.predict import BoxDecoder
    if which == "fixture maps":
        from test_oracle_predict import maps
        probs, deltas = maps()
    else:          # tests/test_gpu_predict.py::test_predict_matches_oracle_random's maps
        seed, dense = which
        rng = np.random.default_rng(seed)
        B, h, w = 2, 200, 176
        probs = (rng.random((B, 2, h, w)) * (1.0 if dense else 0.97)).astype(np.float32)
        deltas = (rng.standard_normal((B, 14, h, w)) * 0.3).astype(np.float32)
        if dense:
            probs[0, 0, 3, 5:9] = 1.0
            probs[1, 1, 7, 7] = 1.0
    dec = BoxDecoder("Car", DEV, anchors=ot.generate_anchors("Car"))
    p, d = _dev(probs), _dev(deltas)
    boxes, scores, counts = dec.decode_device(p, d)
    assert boxes.is_cuda and scores.is_cuda and counts.is_cuda
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and counts.dtype == torch.int32
    B = probs.shape[0]
    assert tuple(boxes.shape) == (B, 20, 7) and tuple(scores.shape) == (B, 20) and tuple(counts.shape) == (B,)
    lb, ls = dec(p, d)
    bh, sh, ch = boxes.cpu().numpy(), scores.cpu().numpy(), counts.cpu().numpy()
    assert ch.tolist() == [len(s) for s in ls]
    for b in range(B):
        assert np.array_equal(bh[b, :ch[b]].view(np.uint32), lb[b].view(np.uint32)), b          # bit-equal
        assert np.array_equal(sh[b, :ch[b]].view(np.uint32), ls[b].view(np.uint32)), b
        assert (bh[b, ch[b]:] == 0).all() and (sh[b, ch[b]:] == 0).all()
    assert ch.sum() > 0


def test_rpn3d_evaluate_runs_the_loop():
    from dataclasses import replace

    from oracle import torch_ref as tr
    from voxelnet_amd import model as M
    from voxelnet_amd import synth
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.evaluate import DetectionEvaluator
    from voxelnet_amd.predict import BoxDecoder
    from voxelnet_amd.targets import generate_anchors
    from voxelnet_amd.voxelize import voxelize_device
    tg = grid_config("Car", H=16, W=24, oy=1.6)
    batches = []
    for k in range(2):
        feats, coords = [], []
        for b in range(2):
            cloud = synth.synth_cloud("Car", k0=150 + 40 * b, seed=500 + 10 * k + b, grid=tg, overflow_frac=0.03)
            fb, cb, _ = voxelize_device(torch.from_numpy(cloud).to(DEV), tg, b, coord_cols=4)
            feats.append(fb)
            coords.append(cb)
        labels = [synth.synth_labels("Car", 3, 40 + 2 * k + b) for b in range(2)]
        batches.append(([f"{2 * k + b:06d}" for b in range(2)], labels, feats, None, coords, None, None))
    before = M.get_precision()
    M.set_precision("bf16")
    try:
        m = M.RPN3D("Car")
        m.load_state_dict(tr.make_state_dict("Car"))
        m.feature_net._grid = replace(m.feature_net._grid, H=16, W=24)
        m = m.to(DEV).train()
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        # the tiny grid's RPN map is 8 x 12: its anchors are that corner of the class's anchor grid
        dec = BoxDecoder("Car", DEV, anchors=generate_anchors("Car")[:8, :12])
        ev = m.evaluate(batches, DEV, decoder=dec)
        assert isinstance(ev, DetectionEvaluator) and m.training and all(mod.training for mod in m.modules())
        out = ev.compute()
        assert set(out) == {"bev", "3d", "n_gt", "n_det"} and out["n_gt"]["all"] == 12
        for metric in ("bev", "3d"):
            assert list(out[metric]) == ["all", "easy", "moderate", "hard"]
            assert all(math.isnan(v) or 0.0 <= v <= 1.0 for v in out[metric].values())
        for k, v in m.state_dict().items():          # running statistics, counters, parameters: untouched
            assert torch.equal(v, state[k]), k
        m.eval()
        own = DetectionEvaluator("Car", DEV, difficulties=("all",))
        assert m.evaluate(batches[:1], DEV, evaluator=own, decoder=dec) is own and not m.training
        assert own.compute()["n_gt"] == {"all": 6}
    finally:
        M.set_precision(before)


def test_cpu_tensors_raise():
    from voxelnet_amd import _lib
    from voxelnet_amd.evaluate import DetectionEvaluator, box_iou_rotated
    a = torch.zeros((2, 7), dtype=torch.float64)
    with pytest.raises(_lib.VoxelnetHipError):
        box_iou_rotated(a, a.to(DEV))
    with pytest.raises(_lib.VoxelnetHipError):
        box_iou_rotated(a.to(DEV), a)
    ev = DetectionEvaluator("Car", DEV)
    with pytest.raises(_lib.VoxelnetHipError):
        ev.update(torch.zeros((1, 20, 7)), torch.zeros((1, 20)), torch.zeros(1, dtype=torch.int32), [[]])
    with pytest.raises(_lib.VoxelnetHipError):
        ev.update(torch.zeros((1, 20, 7), device=DEV), torch.zeros((1, 20)), torch.zeros(1, dtype=torch.int32, device=DEV), [[]])
    assert ev.compute()["n_det"] == 0
