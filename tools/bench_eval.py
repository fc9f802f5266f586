"""The detection-scoring stage alone (csrc/eval.hip, voxelnet_amd/evaluate.py):
  1. `vn_eval_match` per batch — B = 2 and B = 64 frames, top_k = 20 detections, 12 and 128 ground truths per frame, four
     difficulties: time per launch in a back-to-back train of launches (device events), with and without iou_out;
  2. `vn_box_iou_rotated` on 20 x 12 and 20 x 128 pairs, per launch;
  3. `DetectionEvaluator.update` per batch of 2 from device tensors (label parsing, three small uploads, the launch, two
     queued copies): host wall time per call;
  4. the float64 NumPy / Python reference (tests/eval_ref.py) per frame on the host: IoU tables + the eight matchings.
No threshold is set on these numbers: they are there to confirm or refute the estimate that the stage is invisible
beside a 2-3 ms inference.
usage: python tools/bench_eval.py [--out FILE]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd"), os.path.join(ROOT, "tests")]
import numpy as np
import torch
import eval_ref as R
from voxelnet_amd import _lib
from voxelnet_amd.evaluate import DetectionEvaluator, box_iou_rotated

dev = "cuda:0"
TOP_K, N_DIFF = 20, 4
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def train_of_launches(fn, n):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3          # us


def frame(rng, n_gt):
    """n_gt ground truths on a grid (disjoint, car-sized), TOP_K detections: jittered copies of ground truths"""
    gt = np.array([[6.0 + 5.0 * (k % 13), -31.5 + 7.0 * (k // 13), -1.6, 1.5, 1.6, 4.0, 0.3 * ((k % 5) - 2)] for k in range(n_gt)])
    det = gt[rng.integers(0, n_gt, TOP_K)].copy()
    det[:, 0:2] += rng.normal(0, 0.25, (TOP_K, 2))
    det[:, 6] += rng.normal(0, 0.1, TOP_K)
    det[:, 3:6] *= rng.uniform(0.93, 1.07, (TOP_K, 3))
    flags = rng.random((N_DIFF, n_gt)) < 0.3
    scores = (0.96 + 0.04 * rng.random(TOP_K)).astype(np.float32)
    return det.astype(np.float32), scores, gt, flags


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


say("== vn_eval_match: us per launch in a train of 300 launches (top_k 20, 4 difficulties, both metrics) ==")
rng = np.random.default_rng(0)
host_frames = {}
for n_gt in (12, 128):
    for B in (2, 64):
        fr = [frame(rng, n_gt) for _ in range(B)]
        host_frames[n_gt] = fr[:2]
        det, sc = up(np.stack([f[0] for f in fr])), up(np.stack([f[1] for f in fr]))
        dc = up(np.full(B, TOP_K, dtype=np.int32))
        gt, gc = up(np.stack([f[2] for f in fr])), up(np.full(B, n_gt, dtype=np.int32))
        fl = up(np.stack([f[3] for f in fr]).astype(np.uint8))
        status = torch.empty((B, 2, N_DIFF, TOP_K), dtype=torch.int8, device=dev)
        matched = torch.empty((B, 2, N_DIFF, TOP_K), dtype=torch.int32, device=dev)
        iou = torch.empty((B, 2, TOP_K, n_gt), dtype=torch.float64, device=dev)
        nbytes = _lib.load().vn_eval_match_workspace_bytes(B, TOP_K, n_gt)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        for with_iou in (False, True):
            fn = lambda: _lib.call("vn_eval_match", det.data_ptr(), sc.data_ptr(), dc.data_ptr(), gt.data_ptr(), gc.data_ptr(),  # noqa: E731
                                   fl.data_ptr(), B, TOP_K, n_gt, N_DIFF, 0.7, 0.7, status.data_ptr(), matched.data_ptr(),
                                   iou.data_ptr() if with_iou else None, ws.data_ptr(), nbytes, _lib.raw_stream())
            us = train_of_launches(fn, 300)
            say(f"B = {B:2d}  {n_gt:3d} ground truths ({TOP_K * n_gt:4d} pairs / frame)  iou_out {'yes' if with_iou else 'no ':3s}: "
                f"{us:8.2f} us / launch = {us / B:7.2f} us / frame")

say("== vn_box_iou_rotated: us per launch in a train of 300 launches ==")
for n_gt in (12, 128):
    det, _, gt, _ = host_frames[n_gt][0]
    a, b = up(det.astype(np.float64)), up(gt)
    for metric in ("bev", "3d"):
        us = train_of_launches(lambda: box_iou_rotated(a, b, metric), 300)
        say(f"20 x {n_gt:3d} pairs, {metric:3s}: {us:8.2f} us / call (allocation of the output included)")

say("== DetectionEvaluator.update: host wall time per batch of 2 (device tensors in; 12 ground truths per frame) ==")
labels = [[R.label_line("Car", g, 0.0, 0, 50.0) for g in f[2]] for f in host_frames[12]]
det = up(np.stack([f[0] for f in host_frames[12]]))
sc = up(np.stack([f[1] for f in host_frames[12]]))
dc = up(np.full(2, TOP_K, dtype=np.int32))
ev = DetectionEvaluator("Car", dev)
for _ in range(20):
    ev.update(det, sc, dc, labels)
ev.compute()
ev.reset()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(200):
    ev.update(det, sc, dc, labels)
t1 = time.perf_counter()
out = ev.compute()
t2 = time.perf_counter()
say(f"update: {(t1 - t0) / 200 * 1e3:6.3f} ms / batch of 2 (enqueue only, nothing waited for);  compute() over 400 frames / "
    f"{out['n_det']} detections: {(t2 - t1) * 1e3:6.2f} ms")

say("== float64 NumPy / Python reference on the host (tests/eval_ref.py): ms per frame, IoU tables + 8 matchings ==")
for n_gt in (12, 128):
    ts = []
    for det, scores, gt, flags in host_frames[n_gt]:
        for _ in range(3 if n_gt == 12 else 1):
            t0 = time.perf_counter()
            d64 = det.astype(np.float64)
            both = np.zeros((2, TOP_K, n_gt))
            for i in range(TOP_K):
                for j in range(n_gt):
                    both[:, i, j] = R.iou_pair(d64[i], gt[j])
            for m in range(2):
                for k in range(N_DIFF):
                    R.match_frame(both[m], scores, flags[k], 0.7)
            ts.append(time.perf_counter() - t0)
    say(f"{TOP_K} x {n_gt:3d} pairs: {np.mean(ts) * 1e3:8.2f} ms / frame")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")
