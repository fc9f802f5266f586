"""The evaluation tail alone (csrc/detect.hip) on the full car grid, N = 70,400 anchors, B = 2:
  1. `vn_rpn_predict` (the reference's tail: 20 candidates, stand-up NMS) per launch, at score thresholds that leave about
     1 k, 10 k and all 70,400 candidates per sample;
  2. `vn_rpn_detect` per launch for pre_top_k in {20, 1024, 4096} x {stand-up, rotated} x the same thresholds (NMS at 0.1,
     post-NMS cap 20), and its two halves `vn_rpn_select_decode` / `vn_box_nms` at the predict.EVAL_DECODE preset;
  3. the eval-mode bf16 forward of RPN3D (batch 2, synthetic clouds) in the same process, for the ratio.
Times are per launch in a back-to-back train of launches (device events).  The maps are uniform random scores and 0.3-sigma
deltas: boxes of neighbouring anchors overlap heavily, as a trained head's do.  No threshold is set on these numbers.
usage: python tools/bench_detect.py [--out FILE]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import numpy as np
import torch
from voxelnet_amd import _lib
from voxelnet_amd import model as M
from voxelnet_amd import synth
from voxelnet_amd.config import grid_config
from voxelnet_amd.predict import EVAL_DECODE, BoxDecoder, nms_device
from voxelnet_amd.voxelize import voxelize_device

dev = "cuda:0"
B, POST, NMS_THRES = 2, 20, 0.1
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def train_of_launches(fn, n):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3          # us


dec = BoxDecoder("Car", dev)
N = dec.n_anchors
rng = np.random.default_rng(0)
probs = torch.from_numpy(rng.random((B, 2, 200, 176)).astype(np.float32)).to(dev)
deltas = torch.from_numpy((rng.standard_normal((B, 14, 200, 176)) * 0.3).astype(np.float32)).to(dev)
boxes = torch.zeros((B, 64, 7), dtype=torch.float32, device=dev)
scores = torch.zeros((B, 64), dtype=torch.float32, device=dev)
counts = torch.zeros(B, dtype=torch.int32, device=dev)
lib = _lib.load()
THRESHOLDS = [(1.0 - 1000.0 / N, "~1 k"), (1.0 - 10000.0 / N, "~10 k"), (0.0, "70,400")]

say(f"== vn_rpn_predict (top_k {POST}, stand-up): us per launch in a train of 100 launches, N = {N}, B = {B} ==")
nb = lib.vn_rpn_predict_workspace_bytes(B, N)
ws = torch.empty(nb, dtype=torch.uint8, device=dev)
for thres, what in THRESHOLDS:
    us = train_of_launches(lambda: _lib.call("vn_rpn_predict", probs.data_ptr(), deltas.data_ptr(), dec._anchors_dev.data_ptr(), B, N,
                                             thres, NMS_THRES, POST, dec.anchor_h, boxes.data_ptr(), scores.data_ptr(),
                                             counts.data_ptr(), ws.data_ptr(), nb, _lib.raw_stream()), 100)
    say(f"{what:>7s} candidates / sample: {us:9.1f} us / launch")

say(f"== vn_rpn_detect (NMS at {NMS_THRES}, post-NMS cap {POST}): us per launch in a train of 100 launches ==")
for pre in (20, 1024, 4096):
    nb = lib.vn_rpn_detect_workspace_bytes(B, N, pre)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    for mode, name in ((_lib.VN_NMS_STANDUP, "stand-up"), (_lib.VN_NMS_ROTATED, "rotated")):
        for thres, what in THRESHOLDS:
            us = train_of_launches(lambda: _lib.call("vn_rpn_detect", probs.data_ptr(), deltas.data_ptr(), dec._anchors_dev.data_ptr(),
                                                     B, N, thres, pre, mode, NMS_THRES, POST, dec.anchor_h, boxes.data_ptr(),
                                                     scores.data_ptr(), counts.data_ptr(), ws.data_ptr(), nb, _lib.raw_stream()), 100)
            torch.cuda.synchronize()
            say(f"pre_top_k {pre:4d}  {name:8s}  {what:>7s} candidates / sample: {us:9.1f} us / launch   (kept {counts.tolist()})")

say(f"== the preset predict.EVAL_DECODE = {EVAL_DECODE}, cap {POST}: the two halves, Python wrappers (allocations included) ==")
pre = EVAL_DECODE["pre_nms_top_k"]
us_sel = train_of_launches(lambda: dec.candidates_device(probs, deltas, EVAL_DECODE["score_thres"], pre), 100)
cb, _, _, cc = dec.candidates_device(probs, deltas, EVAL_DECODE["score_thres"], pre)
us_nms = train_of_launches(lambda: nms_device(cb, cc, EVAL_DECODE["nms"], EVAL_DECODE["nms_thres"], POST), 100)
us_all = train_of_launches(lambda: dec.decode_device(probs, deltas, top_k=POST, **EVAL_DECODE), 100)
us_old = train_of_launches(lambda: dec.decode_device(probs, deltas, top_k=POST), 100)
say(f"candidates_device {us_sel:9.1f} us   nms_device {us_nms:9.1f} us   decode_device(**EVAL_DECODE) {us_all:9.1f} us   "
    f"decode_device() as before {us_old:9.1f} us")

say("== eval-mode forward, bf16, car grid, batch 2 (synthetic clouds, ~6000 voxels each): ms per forward ==")
g = grid_config("Car")
feats, coords = [], []
for b in range(B):
    cloud = synth.synth_cloud("Car", k0=6000, seed=100 + b)
    fb, cb_, _ = voxelize_device(torch.from_numpy(cloud).to(dev), g, b, coord_cols=4)
    feats.append(fb)
    coords.append(cb_)
M.set_precision("bf16")
m = M.RPN3D("Car").to(dev).eval()


def forward():
    with torch.no_grad():
        return m.detect(feats, coords)


us_fwd = train_of_launches(forward, 30)
prob, delta = forward()
us_tail = train_of_launches(lambda: dec.decode_device(prob, delta, top_k=POST, **EVAL_DECODE), 100)
us_tail_old = train_of_launches(lambda: dec.decode_device(prob, delta, top_k=POST), 100)
say(f"forward {us_fwd / 1e3:7.3f} ms;  on ITS maps (untrained head): decode_device(**EVAL_DECODE) {us_tail / 1e3:7.3f} ms, "
    f"decode_device() as before {us_tail_old / 1e3:7.3f} ms")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")
