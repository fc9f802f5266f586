"""GPU: image-plane scoring (csrc/eval.hip through vn_boxes_to_image / vn_eval_match_image, voxelnet_amd/evaluate.py's
KittiDetectionEvaluator, RPN3D.evaluate(calib=...)) against the float64 restatement tests/kitti_ref.py (DESIGN.md section
1b-bis).

Bars.  Image rows, similarity, iou_out: |device - reference| <= 1e-9 absolute — section 1b's bar for float64 device
arithmetic; the quantities are <= 1242 px, <= 100 m, or radians, so 1e-9 is >= 4e3 ulp of the largest of them.  status,
matched_gt and the on-image bytes: exact, after the guards below have been asserted ON THE REFERENCE ALONE (conditions on
the inputs; the seeds were chosen on the CPU so that they hold; nothing is skipped at run time): no IoU of any metric
within 1e-6 of its threshold, no DontCare overlap within 1e-6 of 0.5, no height within 1e-6 of a bar, no corner depth
within 1e-6 of 0.1, no clipped extent within 1e-6 of 0, no angle within 1e-6 of the wrap seam.  AP / AOS: 1e-12."""
import functools
import math

import numpy as np
import pytest
import torch

import kitti_ref as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-9
MARGIN = 1e-6
SEEDS = (0, 1, 2, 3)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------ inputs
def _frame(det, scores, lines, calib=K.MEAN_CALIB, image_hw=K.IMAGE_HW):
    det = np.asarray(det, dtype=np.float64).reshape(-1, 7).astype(np.float32)
    return {"det": det, "scores": np.asarray(scores, dtype=np.float32).reshape(-1), "lines": list(lines), "calib": calib,
            "image_hw": image_hw}


def _with_height(box, want):
    """the box with its h chosen (bisection, on the CPU) so that its projected 2D height under the mean calibration is
    `want` px as a float32 detection"""
    lo, hi = 0.5, 3.0
    for _ in range(60):
        mid = (lo + hi) / 2
        b = np.array(box, dtype=np.float64)
        b[3] = mid
        row = K.project_box(b.astype(np.float32))["row"]
        lo, hi = (mid, hi) if row[4] - row[2] < want else (lo, mid)
    b[3] = hi
    return b


def _grid_gts(n=128):
    out = []
    for k in range(n):
        i, j = k % 13, k // 13
        out.append([6.0 + 5.0 * i, -31.5 + 7.0 * j, -1.6, 1.5, 1.6, 4.0, 0.3 * ((k % 5) - 2)])
    return np.array(out, dtype=np.float64)


def _jitter(rng, g, s=0.15):
    d = np.array(g, dtype=np.float64)
    d[0:2] += rng.normal(0, s, 2)
    d[2] += rng.normal(0, 0.05)
    d[6] += rng.normal(0, 0.05)
    d[3:6] *= rng.uniform(0.95, 1.05, 3)
    return d


def _grown(box, margin, calib=K.MEAN_CALIB):
    x1, y1, x2, y2 = K.project_box(np.asarray(box, dtype=np.float32), calib)["row"][1:5]
    return [x1 - margin, y1 - margin, x2 + margin, y2 + margin]


HAND = ("limits", "no detections", "no ground truths", "off the image", "corner behind the camera", "cut by the border",
        "dontcare", "height bar")


def _hand_frames():
    rng = np.random.default_rng(77)
    car = [20.0, 3.0, -1.6, 1.5, 1.6, 4.0, 0.2]
    three = [car, [30.0, -8.0, -1.6, 1.5, 1.6, 4.0, -1.0], [44.0, 12.0, -1.5, 1.6, 1.7, 4.2, 1.3]]
    frames = []
    # the limits: 32 detections x 128 ground truths x 64 DontCare regions, own calibration
    calib = K.perturbed_calib(rng)
    grid = _grid_gts(128)
    lines = [K.label_line("Van" if k % 7 == 3 else "Car", g, calib, occ=k % 3, trunc=0.1 * (k % 4), digits=6) for k, g in enumerate(grid)]
    on = [k for k, g in enumerate(grid) if K.project_box(g, calib)["on"]]
    det = [_jitter(rng, grid[k]) for k in on[:26]] + [_jitter(rng, grid[k]) for k in (0, 12, 127, 65)] + \
          [[40.0, 1.0, -1.78, 1.56, 1.6, 3.9, 0.0], [33.0, -3.0, -1.78, 1.56, 1.6, 3.9, 1.5]]
    for j in range(64):
        x1, y1 = rng.uniform(0, 1100), rng.uniform(120, 260)
        lines.append(K.dontcare_line([x1, y1, x1 + rng.uniform(10, 120), y1 + rng.uniform(10, 50)]))
    lines[-1] = K.dontcare_line(_grown(det[-1], 3.0, calib))          # the last region of 64 decides a detection
    frames.append(_frame(det, 0.96 + 0.001 * rng.permutation(32), lines, calib))
    # no detections; no ground truths (one DontCare region, on a detection)
    frames.append(_frame(np.zeros((0, 7)), [], [K.label_line("Car", g) for g in three]))
    det = [_jitter(rng, g) for g in three]
    frames.append(_frame(det, [0.99, 0.98, 0.97], [K.dontcare_line(_grown(det[1], 2.0)), K.label_line("Tram", car)]))
    # every detection off the image: behind the car, far to the side, above the image, and a degenerate box
    det = [[-15.0, 0.0, -1.6, 1.5, 1.6, 4.0, 0.2], [30.0, 35.0, -1.7, 1.5, 1.6, 3.9, 0.0], [12.0, -25.0, -1.6, 1.5, 1.6, 4.0, 0.4],
           [20.0, 0.0, 9.0, 1.5, 1.6, 4.0, 0.0], [20.0, 3.0, -1.6, 1.5, 0.0, 4.0, 0.2]]
    frames.append(_frame(det, [0.99, 0.98, 0.97, 0.965, 0.961], [K.label_line("Car", g) for g in three]))
    # a corner behind the camera: the centre is in front of it, the near corners are not
    det = [[1.9, 0.0, -1.7, 1.5, 1.6, 3.9, 0.0], [0.8, 0.3, -1.7, 1.5, 1.6, 3.9, 0.3], _jitter(rng, car)]
    frames.append(_frame(det, [0.99, 0.98, 0.97], [K.label_line("Car", g) for g in three] +
                         [K.label_line("Car", [1.9, 0.0, -1.7, 1.5, 1.6, 3.9, 0.0])]))
    # boxes cut by the image border: left, right and bottom; their ground truths carry the cut 2D box
    cut = [[10.0, 7.6, -1.7, 1.5, 1.6, 3.9, 0.1], [12.0, -9.0, -1.7, 1.5, 1.6, 3.9, -0.2], [4.6, 0.5, -1.8, 1.5, 1.6, 3.9, 0.05]]
    frames.append(_frame([_jitter(rng, g, 0.08) for g in cut], [0.99, 0.98, 0.97], [K.label_line("Car", g, digits=6) for g in cut]))
    # DontCare: a TP inside a region stays TP, an FP wholly inside one -> IGNORED, an FP 40 % inside one stays FP
    tp, fp_in, fp_40 = _jitter(rng, car, 0.05), [35.0, -6.0, -1.78, 1.56, 1.6, 3.9, 0.0], [28.0, 8.0, -1.78, 1.56, 1.6, 3.9, 1.5]
    x1, y1, x2, y2 = _grown(fp_40, 0.0)
    lines = [K.label_line("Car", car, digits=6), K.dontcare_line(_grown(tp, 4.0)), K.dontcare_line(_grown(fp_in, 1.0)),
             K.dontcare_line([x1 - 10, y1 - 10, x1 + 0.4 * (x2 - x1), y2 + 10])]
    frames.append(_frame([tp, fp_in, fp_40], [0.99, 0.98, 0.97], lines))
    # a 24-px and a 26-px detection on the same ground truth; the 24-px one has the better score
    far = [47.0, 2.0, -1.6, 1.5, 1.6, 4.0, 0.2]
    lines = [K.label_line("Car", far, bbox=[0, 0, 0, 0], digits=6)]
    gt_bb = K.project_box(far)["row"][1:5].copy()
    gt_bb[3] = gt_bb[1] + 26.5
    lines = [K.label_line("Car", far, bbox=gt_bb, digits=6)]
    frames.append(_frame([_with_height(far, 24.0), _with_height(far, 26.0)], [0.99, 0.98], lines))
    assert len(frames) == len(HAND)
    return frames


@functools.lru_cache(maxsize=None)
def _frames(name):
    if name == "hand":
        return _hand_frames()
    return [_frame(f["det"], f["scores"], f["lines"], f["calib"], f["image_hw"]) for f in K.make_scene(int(name))]


@functools.lru_cache(maxsize=None)
def _reference(name, thr, bars=None, mean_projection=False):
    """the reference's answer per frame, computed once and shared (never modified).  bars: the height bars (None: the
    protocol's); mean_projection: the detections are projected with the mean calibration instead of the frame's own"""
    out = []
    for f in _frames(name):
        gt = K.frame_ground_truth(f["lines"], "Car", K.DIFFS, f["calib"])
        r = K.evaluate_frame(f["det"], f["scores"], gt, K.MEAN_CALIB if mean_projection else f["calib"], f["image_hw"], K.DIFFS,
                             (thr, thr, thr), bars)
        r["gt"] = gt
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(r)
    return out


def _assert_guards(frames, refs, thrs):
    """the preconditions, on the reference alone"""
    near = {"iou": 1.0, "dontcare": 1.0, "height": 1.0, "depth": 1.0, "extent": 1.0, "seam": 1.0}
    for f, r in zip(frames, refs):
        for v in r["iou"].reshape(-1):
            near["iou"] = min([near["iou"]] + [abs(float(v) - t) for t in thrs])
        for d in range(len(f["det"])):
            if r["depths"][d] is not None:
                near["depth"] = min(near["depth"], float(np.abs(r["depths"][d] - 0.1).min()))
                near["seam"] = min([near["seam"]] + [K.seam_distance(a) for a in r["angles"][d]])
            if r["raw"][d] is not None:
                x1, y1, x2, y2 = r["raw"][d]
                near["extent"] = min(near["extent"], abs(x2 - x1), abs(y2 - y1))
            if r["on"][d]:
                near["dontcare"] = min(near["dontcare"], abs(float(r["dc_overlap"][d]) - 0.5))
                near["height"] = min([near["height"]] + [abs(float(r["heights"][d]) - b) for b in (25.0, 40.0)])
        for line in f["lines"]:
            if line.split()[0] in ("Car", "Van"):
                near["seam"] = min(near["seam"], K.seam_distance(-float(line.split()[14]) - math.pi / 2))
    for what, v in near.items():
        assert v > MARGIN, f"{what}: an input lies {v:.2e} from a decision boundary: choose other inputs"
    return near


# -------------------------------------------------------------------------------------------------- device run
def _arrays(frames, refs, top_k):
    B, n_diff = len(frames), len(K.DIFFS)
    G = max([len(r["gt"]["boxes"]) for r in refs] + [1])
    D = max(len(r["gt"]["dontcare"]) for r in refs)
    a = {"det": np.zeros((B, top_k, 7), np.float32), "sc": np.zeros((B, top_k), np.float32), "dc": np.zeros(B, np.int32),
         "gt": np.zeros((B, G, 7)), "gc": np.zeros(B, np.int32), "fl": np.zeros((B, n_diff, G), np.uint8), "gb": np.zeros((B, G, 4)),
         "ga": np.zeros((B, G)), "dcb": np.zeros((B, max(D, 1), 4)), "dcc": np.zeros(B, np.int32), "cal": np.zeros((B, 24)),
         "hw": np.zeros((B, 2), np.int32)}
    for b, (f, r) in enumerate(zip(frames, refs)):
        n, g, nd = len(f["det"]), len(r["gt"]["boxes"]), len(r["gt"]["dontcare"])
        a["det"][b, :n], a["sc"][b, :n], a["dc"][b] = f["det"], f["scores"], n
        a["gt"][b, :g], a["gc"][b], a["fl"][b, :, :g] = r["gt"]["boxes"], g, r["gt"]["flags"]
        a["gb"][b, :g], a["ga"][b, :g] = r["gt"]["bbox"], r["gt"]["alpha"]
        a["dcb"][b, :nd], a["dcc"][b] = r["gt"]["dontcare"], nd
        a["cal"][b] = np.concatenate([K.lidar_to_cam(f["calib"])[:3].reshape(-1), np.asarray(f["calib"][0]).reshape(-1)])
        a["hw"][b] = f["image_hw"]
    return a, G, D


def _run(a, G, D, thr, top_k, bars=(0.0, 40.0, 25.0, 25.0), want_iou=True):
    """vn_boxes_to_image + vn_eval_match_image on the arrays as ONE batch -> host arrays"""
    from voxelnet_amd import _lib
    B, n_diff = a["det"].shape[0], len(K.DIFFS)
    d = {k: _dev(v) for k, v in a.items()}
    mh = _dev(np.array(bars, dtype=np.float64))
    rows = torch.full((B, top_k, 12), -7.0, dtype=torch.float64, device=DEV)
    on = torch.full((B, top_k), 9, dtype=torch.uint8, device=DEV)
    status = torch.full((B, 3, n_diff, top_k), 99, dtype=torch.int8, device=DEV)
    matched = torch.full((B, 3, n_diff, top_k), -99, dtype=torch.int32, device=DEV)
    sim = torch.full((B, n_diff, top_k), -7.0, dtype=torch.float64, device=DEV)
    iou = torch.full((B, 3, top_k, G), -1.0, dtype=torch.float64, device=DEV) if want_iou else None
    nbytes = _lib.load().vn_eval_match_workspace_bytes(B, top_k, G)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    s = _lib.raw_stream()
    _lib.call("vn_boxes_to_image", d["det"].data_ptr(), d["dc"].data_ptr(), d["cal"].data_ptr(), d["hw"].data_ptr(), B, top_k,
              rows.data_ptr(), on.data_ptr(), s)
    _lib.call("vn_eval_match_image", d["det"].data_ptr(), d["sc"].data_ptr(), d["dc"].data_ptr(), d["gt"].data_ptr(), d["gc"].data_ptr(),
              d["fl"].data_ptr(), rows.data_ptr(), on.data_ptr(), d["gb"].data_ptr(), d["ga"].data_ptr(),
              d["dcb"].data_ptr() if D else None, d["dcc"].data_ptr() if D else None, mh.data_ptr(), B, top_k, G, D, n_diff,
              float(thr), float(thr), float(thr), status.data_ptr(), matched.data_ptr(), sim.data_ptr(),
              iou.data_ptr() if want_iou else None, ws.data_ptr(), nbytes, s)
    torch.cuda.synchronize()
    order = ws.cpu().numpy()[:B * top_k * 4].view(np.int32).reshape(B, top_k)
    return {"rows": rows.cpu().numpy(), "on": on.cpu().numpy(), "status": status.cpu().numpy(), "matched": matched.cpu().numpy(),
            "similarity": sim.cpu().numpy(), "iou": iou.cpu().numpy() if want_iou else None, "order": order}


def _compare(frames, refs, got, top_k, what):
    """status / matched_gt / on-image bytes exactly; rows, similarity, iou_out within TOL; padding as documented"""
    worst = {"rows": 0.0, "similarity": 0.0, "iou": 0.0}
    for b, (f, r) in enumerate(zip(frames, refs)):
        n, g = len(f["det"]), len(r["gt"]["boxes"])
        assert np.array_equal(got["on"][b, :n], r["on"].astype(np.uint8)), (what, b)
        assert (got["on"][b, n:] == 0).all() and (got["rows"][b, n:] == 0).all(), (what, b)          # past the count: zeros
        assert (got["rows"][b, :n][~r["on"]][:, 1:5] == 0).all(), (what, b)                            # off the image: no 2D box
        assert np.array_equal(got["status"][b, :, :, :n], r["status"]), (what, b, got["status"][b, :, :, :n], r["status"])
        assert np.array_equal(got["matched"][b, :, :, :n], r["matched"]), (what, b)
        assert (got["status"][b, :, :, n:] == -2).all() and (got["matched"][b, :, :, n:] == -1).all(), (what, b)
        assert (got["similarity"][b, :, n:] == 0).all(), (what, b)
        assert got["order"][b, :n].tolist() == sorted(range(n), key=lambda d: (-float(f["scores"][d]), d)), (what, b)
        assert (got["order"][b, n:] == -1).all()
        if n:
            worst["rows"] = max(worst["rows"], float(np.abs(got["rows"][b, :n] - r["rows"]).max()))
            worst["similarity"] = max(worst["similarity"], float(np.abs(got["similarity"][b, :, :n] - r["similarity"]).max()))
        if got["iou"] is not None:
            if n and g:
                worst["iou"] = max(worst["iou"], float(np.abs(got["iou"][b, :, :n, :g] - r["iou"]).max()))
            pad = got["iou"][b].copy()
            pad[:, :n, :g] = 0
            assert (pad == 0).all(), (what, b)
    print(f"{what}: max |device - reference|: rows {worst['rows']:.3e}, similarity {worst['similarity']:.3e}, "
          f"iou_out {worst['iou']:.3e}")
    assert max(worst.values()) <= TOL, worst
    return worst


# ---------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("thr", [0.7, 0.5])
@pytest.mark.parametrize("case", [str(s) for s in SEEDS] + ["hand"])
def test_image_match_vs_reference(case, thr):
    frames, refs = _frames(case), _reference(case, thr)
    near = _assert_guards(frames, refs, (thr,))
    top_k = 32 if case == "hand" else 20
    a, G, D = _arrays(frames, refs, top_k)
    if case == "hand":
        assert (G, D) == (128, 64) and a["dc"][0] == 32
    got = _run(a, G, D, thr, top_k)
    st = np.concatenate([r["status"].reshape(-1) for r in refs])
    print(f"case {case} thr {thr}: {len(frames)} frames, G {G}, D {D}; nearest to a boundary "
          + ", ".join(f"{k} {v:.1e}" for k, v in near.items())
          + f"; TP/FP/ignored {int((st == 1).sum())}/{int((st == 0).sum())}/{int((st == -1).sum())}")
    _compare(frames, refs, got, top_k, f"case {case} thr {thr}")
    got2 = _run(a, G, D, thr, top_k, want_iou=False)          # without the IoU tables asked for: the same answers
    for k in ("status", "matched", "similarity", "rows", "on"):
        assert np.array_equal(got2[k], got[k]), k


def test_hand_frames_do_what_they_were_built_for():
    """the reference's own answers on the hand-made frames are the ones they were built to provoke (so the comparison
    above covers them)"""
    frames, refs = _frames("hand"), _reference("hand", 0.7)
    r = dict(zip(HAND, refs))
    lim = r["limits"]
    assert lim["status"].shape == (3, 4, 32) and len(lim["gt"]["boxes"]) == 128 and len(lim["gt"]["dontcare"]) == 64
    assert (lim["status"] == 1).any() and (lim["matched"] >= 64).any() and lim["gt"]["flags"][0].any()
    assert lim["dc_overlap"][31] > 0.99 and (lim["status"][:, 0, 31] == -1).all()          # decided by the 64th region
    assert r["no detections"]["status"].shape == (3, 4, 0)
    assert (r["no ground truths"]["status"][:, 0] == [0, -1, 0]).all()          # (one of them sits in the DontCare region)
    off = r["off the image"]
    assert not off["on"].any() and (off["status"] == -1).all() and (off["matched"] == -1).all()
    assert off["depths"][0].max() < 0 and off["depths"][1].min() > 0.1 and off["depths"][4] is None
    cor = r["corner behind the camera"]
    assert cor["on"].tolist() == [False, False, True] and cor["rows"][0, 10] > 0.1 and cor["depths"][0].min() < 0.1
    assert cor["depths"][1].min() < 0 < cor["depths"][1].max()
    assert (cor["status"][:, 0, 0] == -1).all() and (cor["matched"][:, :, 0] == -1).all() and (cor["status"][:, 0, 2] == 1).all()
    cut = r["cut by the border"]
    assert cut["on"].all() and cut["rows"][0, 1] == 0.0 and cut["rows"][1, 3] == K.IMAGE_HW[1] - 1.0 \
        and cut["rows"][2, 4] == K.IMAGE_HW[0] - 1.0
    assert (cut["status"][2, 0] == 1).all()          # the cut 2D boxes still match their ground truths
    dc = r["dontcare"]
    assert dc["dc_overlap"][0] == 1.0 and dc["dc_overlap"][1] == 1.0 and 0.35 < dc["dc_overlap"][2] < 0.45
    assert (dc["status"][:, 0] == [1, -1, 0]).all()
    hb = r["height bar"]
    assert abs(hb["heights"][0] - 24.0) < 0.05 and abs(hb["heights"][1] - 26.0) < 0.05
    assert (hb["iou"][:, :, 0] > 0.7).all()
    assert (hb["status"][:, 0] == [1, 0]).all()          # all: the better score takes the ground truth
    assert (hb["status"][:, 2] == [-1, 1]).all() and (hb["status"][:, 3] == [-1, 1]).all()          # 25-px bar
    assert (hb["status"][:, 1] == [-1, -1]).all() and (hb["matched"][:, 1] == -1).all()             # 40-px bar: both under it


@pytest.mark.parametrize("case", ["0", "2"])
def test_bev_and_3d_equal_vn_eval_match_when_nothing_is_filtered(case):
    """every detection on the image, all bars 0, no DontCare region: the bev / 3d slices are vn_eval_match's, bit for bit"""
    from test_gpu_detection_eval import _run_match
    frames, refs = _frames(case), _reference(case, 0.5)
    kept, kept_refs = [], []
    for f, r in zip(frames, refs):
        on = r["on"]
        kept.append({"det": f["det"][on], "scores": f["scores"][on], "gt": r["gt"]["boxes"], "flags": r["gt"]["flags"],
                     "calib": f["calib"], "image_hw": f["image_hw"]})
        gt = dict(r["gt"])
        gt["dontcare"] = np.zeros((0, 4))
        kept_refs.append({"gt": gt})
    assert sum(len(f["det"]) for f in kept) >= 30
    a, G, D = _arrays(kept, kept_refs, 20)
    assert D == 0
    got = _run(a, G, D, 0.5, 20, bars=(0.0, 0.0, 0.0, 0.0))
    status, matched, iou, order = _run_match(kept, 0.5, 0.5, top_k=20)
    for b, f in enumerate(kept):
        assert got["on"][b, :len(f["det"])].all()
    assert np.array_equal(got["status"][:, :2], status) and np.array_equal(got["matched"][:, :2], matched)
    assert np.array_equal(got["iou"][:, :2].view(np.uint64), iou.view(np.uint64)) and np.array_equal(got["order"], order)
    assert (status == 1).any() and (status == 0).any() and (status == -1).any()


def test_the_frames_calibration_is_read():
    """the same frames with the mean calibration in place of their own for the projection: the device follows the reference
    there too, and at least one status changes"""
    frames, own, mean = _frames("1"), _reference("1", 0.5), _reference("1", 0.5, None, True)
    mean_frames = [dict(f, calib=K.MEAN_CALIB) for f in frames]
    _assert_guards(mean_frames, mean, (0.5,))
    a, G, D = _arrays(frames, own, 20)
    got_own = _run(a, G, D, 0.5, 20)
    a["cal"][:] = np.concatenate([K.lidar_to_cam(K.MEAN_CALIB)[:3].reshape(-1), K.MEAN_P2.reshape(-1)])
    got_mean = _run(a, G, D, 0.5, 20)
    _compare(mean_frames, mean, got_mean, 20, "mean calibration")
    assert not np.array_equal(got_own["status"], got_mean["status"])
    assert np.abs(got_own["rows"] - got_mean["rows"]).max() > 1.0


# ------------------------------------------------------------------------------------------------ AP end to end
@functools.lru_cache(maxsize=None)
def _ap_scene():
    scene = [f for s in SEEDS[:3] for f in _frames(str(s))] + _frames("hand")[1:]
    ref = K.RefEvaluator("Car")
    for f in scene:
        ref.add_frame(f["det"], f["scores"], f["lines"], f["calib"], f["image_hw"])
    return scene, ref, ref.compute()


def _feed(ev, scene, batch, device_form, top_k=20):
    for i in range(0, len(scene), batch):
        part = scene[i:i + batch]
        kw = dict(calibs=[p["calib"] for p in part], image_shapes=[p["image_hw"] for p in part],
                  tags=[f"{i + b:06d}" for b in range(len(part))])
        labels = [p["lines"] for p in part]
        if device_form:
            B = len(part)
            boxes, scores, counts = np.zeros((B, top_k, 7), np.float32), np.zeros((B, top_k), np.float32), np.zeros(B, np.int32)
            for b, p in enumerate(part):
                n = len(p["scores"])
                boxes[b, :n], scores[b, :n], counts[b] = p["det"], p["scores"], n
            ev.update(_dev(boxes), _dev(scores), _dev(counts), labels, **kw)
        else:
            ev.update([p["det"] for p in part], [p["scores"] for p in part], None, labels, **kw)


def _assert_same_result(got, ref):
    assert set(got) == {"bbox", "bev", "3d", "aos", "n_gt", "n_det", "n_ignored"}
    assert got["n_det"] == ref["n_det"] and got["n_gt"] == ref["n_gt"] and got["n_ignored"] == ref["n_ignored"]
    for m in ("bbox", "bev", "3d", "aos"):
        assert list(got[m]) == list(K.DIFFS)
        for d in K.DIFFS:
            assert abs(got[m][d] - ref[m][d]) <= 1e-12, (m, d, got[m][d], ref[m][d])


@pytest.mark.parametrize("batch,device_form", [(5, True), (8, False)])
def test_ap_and_aos_end_to_end(batch, device_form, tmp_path):
    from voxelnet_amd.evaluate import KittiDetectionEvaluator
    scene, ref_ev, ref = _ap_scene()
    assert len(scene) % batch != 0          # (a ragged last batch)
    ev = KittiDetectionEvaluator("Car", DEV)
    assert ev.iou_thres == (0.7, 0.7, 0.7)
    _feed(ev, scene, batch, device_form)
    got = ev.compute()
    print(f"batch {batch} {'device' if device_form else 'list'} form: " + ", ".join(
        f"{m}/{d} {got[m][d]:.6f}" for m in ("bbox", "aos", "bev", "3d") for d in K.DIFFS)
        + f"; n_gt {got['n_gt']}, n_det {got['n_det']}, n_ignored {got['n_ignored']}")
    _assert_same_result(got, ref)
    assert all(0 < got["aos"][d] < got["bbox"][d] < 1 for d in K.DIFFS) and 0 < got["bev"]["all"] < 1
    assert got["n_ignored"]["all"] > 0 and got["n_ignored"]["easy"] > got["n_ignored"]["hard"] > got["n_ignored"]["all"]
    _assert_same_result(ev.compute(), ref)          # compute() twice
    # the result lines: per frame, the on-image detections in score order, the reference's fields to two decimals
    tags, lines = ev.result_lines()
    assert tags == [f"{i:06d}" for i in range(len(scene))] and len(lines) == len(scene)
    for f, r, ls in zip(scene, ref_ev.frames, lines):
        idx = sorted([d for d in range(len(f["det"])) if r["on"][d]], key=lambda d: (-float(f["scores"][d]), d))
        assert len(ls) == len(idx)
        for line, d in zip(ls, idx):
            fields = line.split()
            assert fields[:3] == ["Car", "-1", "-1"] and len(fields) == 16 and fields[15] == "%.4f" % f["scores"][d]
            assert np.abs(np.array(fields[3:15], dtype=np.float64) - r["rows"][d]).max() <= 0.005 + 1e-8
    paths = ev.write_results(str(tmp_path / "out"))
    assert [p.split("/")[-1] for p in paths] == [t + ".txt" for t in tags]
    for p, ls in zip(paths, lines):
        assert open(p).read() == "".join(l + "\n" for l in ls)
    assert any(not ls for ls in lines)          # (a frame without detections: an empty file)
    ev.reset()
    empty = ev.compute()
    assert empty["n_det"] == 0 and math.isnan(empty["aos"]["all"]) and ev.result_lines() == ([], [])


def test_other_thresholds_classes_and_mean_calibration():
    """thresholds per metric, R11, two difficulties, calibs=None (the mean calibration), Pedestrian's neighbour class"""
    from voxelnet_amd.evaluate import KittiDetectionEvaluator
    rng = np.random.default_rng(5)
    scene = []
    for k in range(6):
        gts = [[rng.uniform(6, 40), rng.uniform(-6, 6), -1.5, 1.73, 0.6, 0.8, rng.uniform(-3, 3)] for _ in range(4)]
        lines = [K.label_line("Person_sitting" if i == 1 else "Pedestrian", g, occ=i % 3, digits=6) for i, g in enumerate(gts)]
        det = [_jitter(rng, g, 0.05) for g in gts] + [[rng.uniform(6, 40), rng.uniform(-6, 6), -1.5, 1.73, 0.6, 0.8, 0.3]]
        lines.append(K.dontcare_line(_grown(det[-1], 2.0)) if k % 2 else K.label_line("Car", gts[0]))
        scene.append(_frame(det, 0.9 + 0.01 * rng.permutation(5), lines))
    diffs, thr = ("hard", "all"), (0.5, 0.25, 0.6)
    ref = K.RefEvaluator("Pedestrian", diffs, thr, recall_points=11)
    for f in scene:
        r = ref.add_frame(f["det"], f["scores"], f["lines"])
        assert min(abs(float(v) - t) for m, t in enumerate(thr) for v in r["iou"][m].reshape(-1)) > MARGIN
        assert np.abs(r["dc_overlap"] - 0.5).min() > MARGIN and np.abs(r["heights"] - 25.0).min() > MARGIN
    ev = KittiDetectionEvaluator("Pedestrian", DEV, iou_thres=thr, difficulties=diffs, recall_points=11)
    ev.update([f["det"] for f in scene], [f["scores"] for f in scene], None, [f["lines"] for f in scene])
    got, want = ev.compute(), ref.compute()
    assert got["n_gt"] == want["n_gt"] and got["n_det"] == want["n_det"] == 30 and got["n_ignored"] == want["n_ignored"]
    for m in ("bbox", "bev", "3d", "aos"):
        for d in diffs:
            assert abs(got[m][d] - want[m][d]) <= 1e-12, (m, d)
    assert got["n_gt"]["all"] == 18 and got["n_ignored"]["all"] == 3 and got["bbox"]["all"] > 0.5
    assert ev.result_lines()[0] == [f"{i:06d}" for i in range(6)]


# ---------------------------------------------------------------------------------------------- RPN3D.evaluate
def test_rpn3d_evaluate_with_and_without_calib(tmp_path):
    from dataclasses import replace

    from oracle import torch_ref as tr
    from test_kitti_eval_host import CALIB_TEXT
    from voxelnet_amd import model as M
    from voxelnet_amd import synth
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.evaluate import DetectionEvaluator, KittiDetectionEvaluator, load_kitti_calib
    from voxelnet_amd.predict import BoxDecoder
    from voxelnet_amd.targets import generate_anchors, label_to_gt_box_3d
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
    tags = [t for x in batches for t in x[0]]
    cdir = tmp_path / "calib"
    cdir.mkdir()
    for t in tags:
        (cdir / f"{t}.txt").write_text(CALIB_TEXT)
    before = M.get_precision()
    M.set_precision("bf16")
    try:
        m = M.RPN3D("Car")
        m.load_state_dict(tr.make_state_dict("Car"))
        m.feature_net._grid = replace(m.feature_net._grid, H=16, W=24)
        m = m.to(DEV).eval()
        dec = BoxDecoder("Car", DEV, anchors=generate_anchors("Car")[:8, :12])
        # without calib: the parent's loop — the same keys and the same values as that loop written out by hand
        ev = m.evaluate(batches, DEV, decoder=dec)
        assert type(ev) is DetectionEvaluator
        out = ev.compute()
        by_hand = DetectionEvaluator("Car", DEV)
        dets = []
        with torch.no_grad():
            for x in batches:
                prob, delta = m.detect(M._parts_to(x[2], DEV), M._parts_to(x[4], DEV))
                dets.append(dec.decode_device(prob, delta, top_k=20))
                by_hand.update(*dets[-1], x[1])
        want = by_hand.compute()
        assert set(out) == {"bev", "3d", "n_gt", "n_det"} and out["n_gt"] == want["n_gt"] and out["n_det"] == want["n_det"]
        for metric in ("bev", "3d"):
            for d, v in out[metric].items():
                assert v == want[metric][d] or (math.isnan(v) and math.isnan(want[metric][d]))
        n_det = [int(c) for det in dets for c in det[2].cpu().numpy()]
        # with calib: a directory, a callable, "mean"
        seen = []
        for calib in (str(cdir), lambda t: seen.append(t) or load_kitti_calib(str(cdir / f"{t}.txt")), "mean"):
            kev = m.evaluate(batches, DEV, decoder=dec, calib=calib)
            assert type(kev) is KittiDetectionEvaluator
            res = kev.compute()
            assert set(res) == {"bbox", "bev", "3d", "aos", "n_gt", "n_det", "n_ignored"}
            assert res["n_gt"]["all"] == 12 and res["n_det"] == sum(n_det)
            paths = kev.write_results(str(tmp_path / "results"))
            assert [p.split("/")[-1] for p in paths] == [t + ".txt" for t in tags]
            for p, n in zip(paths, n_det):
                lines = open(p).read().splitlines()
                assert len(lines) <= n
                for line in lines:
                    f = line.split()
                    assert len(f) == 16 and f[0] == "Car" and 0.0 <= float(f[15]) <= 1.0 and float(f[6]) > float(f[4])
                    assert label_to_gt_box_3d([[" ".join(f[:15])]], "Car")[0].shape == (1, 7)
        assert seen == tags
        own = KittiDetectionEvaluator("Car", DEV, difficulties=("all",))
        assert m.evaluate(batches[:1], DEV, evaluator=own, decoder=dec, calib="mean") is own and not m.training
        assert own.compute()["n_gt"] == {"all": 6}
        with pytest.raises(ValueError):
            m.evaluate(batches[:1], DEV, evaluator=DetectionEvaluator("Car", DEV), decoder=dec, calib="mean")
    finally:
        M.set_precision(before)


def test_cpu_tensors_raise_and_sizes_are_checked():
    from voxelnet_amd import _lib
    from voxelnet_amd.evaluate import KittiDetectionEvaluator
    ev = KittiDetectionEvaluator("Car", DEV)
    with pytest.raises(_lib.VoxelnetHipError):
        ev.update(torch.zeros((1, 20, 7)), torch.zeros((1, 20)), torch.zeros(1, dtype=torch.int32), [[]])
    with pytest.raises(_lib.VoxelnetHipError):
        ev.update(torch.zeros((1, 20, 7), device=DEV), torch.zeros((1, 20)), torch.zeros(1, dtype=torch.int32, device=DEV), [[]])
    with pytest.raises(_lib.VoxelnetHipError):          # 65 DontCare regions
        ev.update([np.zeros((0, 7), np.float32)], [np.zeros(0, np.float32)], None, [[K.dontcare_line([0, 0, 5, 5])] * 65])
    assert ev.compute()["n_det"] == 0
    # the library refuses out-of-range sizes before any launch, with real buffers too
    lib = _lib.load()
    buf = torch.zeros(1 << 16, dtype=torch.float64, device=DEV)
    p = buf.data_ptr()
    for B, k, G, D, n in [(1, 33, 12, 0, 4), (1, 20, 129, 0, 4), (1, 20, 12, 65, 4), (1, 20, 12, 0, 9), (1, 0, 12, 0, 4)]:
        assert lib.vn_eval_match_image(*([p] * 13), B, k, G, D, n, 0.7, 0.7, 0.7, p, p, p, None, p, 1 << 16, None) == -1
    assert lib.vn_eval_match_image(*([p] * 13), 1, 20, 12, 0, 4, 0.7, 0.7, 0.7, p, p, p, None, p, 8, None) == -1      # workspace
    assert lib.vn_boxes_to_image(p, p, p, p, 1, 33, p, p, None) == -1
    torch.cuda.synchronize()
