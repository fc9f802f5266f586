"""Time the five target assigners and the two detection layouts (DESIGN.md sections 1h, 1o, 1p), alternated inside one process.

1. Assignment on the full Car grid (70,400 anchors), B = 2, with 8 and with 128 boxes per frame: us per call (every launch
   of the call: vn_rpn_targets' three, vn_rpn_targets_iou's memset + three, vn_rpn_targets_atss' memset + three) for
     reference   vn_rpn_targets (the reference's assignment; its stand-up rectangles are made on the host beforehand)
     standup     vn_rpn_targets_iou, VN_ASSIGN_STANDUP
     rotated     vn_rpn_targets_iou, VN_ASSIGN_ROTATED
     atss        vn_rpn_targets_atss, VN_ASSIGN_ROTATED, top_k = --atss-top-k (9), no stats; its ratio to `rotated` is printed
     simota      vn_rpn_targets_ota, VN_IOU_BEV, q = --ota-q (10), radius 2.5 site pitches, iou_weight 3, no stats, on seeded
                 maps (probs uniform, deltas N(0, 0.3): what a box's candidates predict does not change how many they are);
                 its ratios to `rotated` and `atss` are printed.  Unlike the others it runs AFTER the forward, on the step's
                 dependency chain — hence part 3
   and, from the same run, the encoder's forward (RPN3D.feature_net on the benchmark's two Car frames, bf16 mode) — the
   assigner runs on the targets stream beside it, off the step's dependency chain.
2. The evaluation tail at predict.EVAL_DECODE (pre-NMS 1024, rotated NMS at 0.1, cap 20) on random full-grid maps, B = 2:
     flat            vn_rpn_detect
     site            vn_rpn_detect_layout, VN_DETECT_SITE
     flat + 2 transposes   the two channels-last copies (torch permute + contiguous), then vn_rpn_detect: what the site
                           layout replaces
3. (--train-step) RPN3D.train_step on the benchmark's two Car frames with 6 labelled cars each, bf16 mode, ClipSGD: target_assign
   "simota" against "atss", both on the separate-calls path (forward, backward, step: what "simota" takes; "atss" is driven
   through the same three calls instead of its one-call step), two models alternated round by round, ms per step.
Method of tools/bench_loss.py: per arm and round --round-launches calls back to back between two device events, the arms
alternated round by round; reported: median [min, max] over the rounds.  No threshold is set on these numbers.
--assign-only leaves out the encoder and the evaluation tail (not part 3).
usage: python tools/bench_assign.py [--rounds 20] [--round-launches 50] [--atss-top-k 9] [--ota-q 10] [--assign-only] [--train-step]
       [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import numpy as np
import torch
from voxelnet_amd import _lib, synth
from voxelnet_amd import model as M
from voxelnet_amd import targets as T
from voxelnet_amd.config import grid_config
from voxelnet_amd.predict import EVAL_DECODE, NMS_MODES, BoxDecoder
from voxelnet_amd.voxelize import voxelize_device

dev = "cuda:0"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--round-launches", type=int, default=50)
ap.add_argument("--atss-top-k", type=int, default=9)
ap.add_argument("--ota-q", type=int, default=10)
ap.add_argument("--assign-only", action="store_true")
ap.add_argument("--train-step", action="store_true")
ap.add_argument("--step-rounds", type=int, default=10)
ap.add_argument("--round-steps", type=int, default=10)
ap.add_argument("--out")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_assign.py needs cuda:0 (there is no CPU path to measure)")
if args.rounds < 5 or args.rounds * args.round_launches < 50:
    sys.exit("at least 5 rounds and 50 timed launches per arm")
lib = _lib.load()
st = _lib.raw_stream()
B = 2
cfg = T.CLASS_CFG["Car"]
anchors = torch.from_numpy(np.ascontiguousarray(T.generate_anchors("Car").reshape(-1, 7))).to(dev)
N = anchors.shape[0]
ota_rng = np.random.default_rng(3)
ota_probs = torch.from_numpy(ota_rng.random((B, 2, 200, 176)).astype(np.float32)).to(dev)
ota_deltas = torch.from_numpy((ota_rng.standard_normal((B, 14, 200, 176)) * 0.3).astype(np.float32)).to(dev)
ota_radius = T.OTA_RADIUS_PITCHES * T.site_pitch(T.generate_anchors("Car"))


def boxes_of(n, seed):
    """n cars inside the range, the sizes and yaws of synth.synth_labels"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(4, 66, n), rng.uniform(-36, 36, n), cfg["z"] + rng.uniform(-0.2, 0.2, n),
                     cfg["h"] * rng.uniform(0.9, 1.1, n), cfg["w"] * rng.uniform(0.9, 1.1, n), cfg["l"] * rng.uniform(0.9, 1.1, n),
                     rng.uniform(-1.5, 1.5, n)], axis=1)


def assigner(kind, G):
    frames = [boxes_of(G, 10 * G + b) for b in range(B)]
    gt = torch.from_numpy(np.stack(frames)).to(dev)
    g2 = torch.from_numpy(np.stack([T.gt_standup_boxes(f) for f in frames])).to(dev)
    cnt = torch.full((B,), G, dtype=torch.int32, device=dev)
    pos, neg = (torch.empty((B, N), dtype=torch.float32, device=dev) for _ in range(2))
    tgt = torch.empty((B, N, 7), dtype=torch.float32, device=dev)
    keep = [gt, g2, cnt, pos, neg, tgt]
    if kind == "reference":
        nb = lib.vn_rpn_targets_workspace_bytes(B, N, G)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        a = (anchors.data_ptr(), N, gt.data_ptr(), g2.data_ptr(), cnt.data_ptr(), B, G, cfg["pos_iou"], cfg["neg_iou"], cfg["h"],
             pos.data_ptr(), neg.data_ptr(), tgt.data_ptr(), ws.data_ptr(), nb, st)
        name = "vn_rpn_targets"
    elif kind == "atss":
        nb = lib.vn_rpn_targets_atss_workspace_bytes(B, N, G, args.atss_top_k)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        a = (anchors.data_ptr(), N, gt.data_ptr(), cnt.data_ptr(), B, G, _lib.VN_ASSIGN_ROTATED, args.atss_top_k, cfg["h"],
             pos.data_ptr(), neg.data_ptr(), tgt.data_ptr(), None, None, ws.data_ptr(), nb, st)
        name = "vn_rpn_targets_atss"
    elif kind == "simota":
        nb = lib.vn_rpn_targets_ota_workspace_bytes(B, N, G, args.ota_q)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        a = (anchors.data_ptr(), N, gt.data_ptr(), cnt.data_ptr(), B, G, ota_probs.data_ptr(), ota_deltas.data_ptr(), _lib.VN_IOU_BEV,
             args.ota_q, ota_radius, 3.0, cfg["h"], pos.data_ptr(), neg.data_ptr(), tgt.data_ptr(), None, None, ws.data_ptr(), nb, st)
        name = "vn_rpn_targets_ota"
    else:
        nb = lib.vn_rpn_targets_iou_workspace_bytes(B, N, G)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        a = (anchors.data_ptr(), N, gt.data_ptr(), cnt.data_ptr(), B, G, T.ASSIGN_KINDS[kind], cfg["pos_iou"], cfg["neg_iou"],
             cfg["h"], pos.data_ptr(), neg.data_ptr(), tgt.data_ptr(), None, ws.data_ptr(), nb, st)
        name = "vn_rpn_targets_iou"
    keep.append(ws)
    return (lambda: _lib.call(name, *a)), keep


arms = []
for G in (8, 128):
    for kind in ("reference", "standup", "rotated", "atss", "simota"):
        run, keep = assigner(kind, G)
        arms.append((f"assign {kind}", f"{G} boxes", run, keep))

# the encoder's forward on the benchmark's two Car frames
feats, coords = [], []
if not args.assign_only:
    M.set_precision("bf16")
    model = M.RPN3D("Car").to(dev).eval()
    grid = grid_config("Car")
    for b, cloud in enumerate(synth.workload_frames(1, batch=B)):
        f, c, _ = voxelize_device(torch.from_numpy(cloud).to(dev), grid, b, coord_cols=4)
        feats.append(f)
        coords.append(c)


def encoder():
    with torch.no_grad():
        model.feature_net(feats, coords)


if not args.assign_only:
    arms.append(("encoder forward", f"K = {sum(f.shape[0] for f in feats)}", encoder, None))

# the detection tail
rng = np.random.default_rng(5)
probs = torch.from_numpy(rng.random((B, 2, 200, 176)).astype(np.float32)).to(dev)
deltas = torch.from_numpy((rng.standard_normal((B, 14, 200, 176)) * 0.3).astype(np.float32)).to(dev)
dec = BoxDecoder("Car", dev)
pre, post, thres, nms_thres = EVAL_DECODE["pre_nms_top_k"], 20, EVAL_DECODE["score_thres"], EVAL_DECODE["nms_thres"]
mode = NMS_MODES[EVAL_DECODE["nms"]]
nb = lib.vn_rpn_detect_workspace_bytes(B, N, pre)
dws = torch.empty(nb, dtype=torch.uint8, device=dev)
ob = torch.zeros((B, post, 7), dtype=torch.float32, device=dev)
osc = torch.zeros((B, post), dtype=torch.float32, device=dev)
oc = torch.zeros(B, dtype=torch.int32, device=dev)


def detect(p, d, layout):
    _lib.call("vn_rpn_detect_layout", p.data_ptr(), d.data_ptr(), dec._anchors_dev.data_ptr(), B, N, thres, pre, mode, nms_thres, post,
              dec.anchor_h, ob.data_ptr(), osc.data_ptr(), oc.data_ptr(), dws.data_ptr(), nb, st, layout)


def flat_with_transposes():
    detect(probs.permute(0, 2, 3, 1).contiguous(), deltas.permute(0, 2, 3, 1).contiguous(), _lib.VN_DETECT_FLAT)


if not args.assign_only:
    arms.append(("detect flat", f"pre {pre}", lambda: detect(probs, deltas, _lib.VN_DETECT_FLAT), None))
    arms.append(("detect site", f"pre {pre}", lambda: detect(probs, deltas, _lib.VN_DETECT_SITE), None))
    arms.append(("detect flat + 2 transposes", f"pre {pre}", flat_with_transposes, None))

for _, _, run, _ in arms:                              # warm-up: code objects, the caches
    for _ in range(10):
        run()
torch.cuda.synchronize()
us = {(a, b): [] for a, b, *_ in arms}
for _ in range(args.rounds):
    for a, b, run, _ in arms:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(args.round_launches):
            run()
        e.record()
        torch.cuda.synchronize()
        us[(a, b)].append(s.elapsed_time(e) / args.round_launches * 1e3)

say(f"== target assignment (full Car grid, {N} anchors, B = {B}) and the evaluation tail: {args.rounds} alternated rounds of "
    f"{args.round_launches} calls per arm; us per call, median [min, max] over the rounds ==")
for a, b, *_ in arms:
    v = us[(a, b)]
    say(f"{a:28s} {b:12s} {statistics.median(v):9.2f} [{min(v):8.2f}, {max(v):8.2f}]")
for G in (8, 128):
    r, t = statistics.median(us[("assign rotated", f"{G} boxes")]), statistics.median(us[("assign atss", f"{G} boxes")])
    say(f"atss (top_k {args.atss_top_k}) / rotated at {G} boxes: {t:.2f} / {r:.2f} = {t / r:.2f}")
    o = statistics.median(us[("assign simota", f"{G} boxes")])
    say(f"simota (q {args.ota_q}) / rotated at {G} boxes: {o:.2f} / {r:.2f} = {o / r:.2f};  / atss: {o:.2f} / {t:.2f} = {o / t:.2f}")

if args.train_step:
    from voxelnet_amd.optim import ClipSGD
    M.set_precision("bf16")
    grid = grid_config("Car")
    sf, sc = [], []
    for b, cloud in enumerate(synth.workload_frames(1, batch=B)):
        f, c, _ = voxelize_device(torch.from_numpy(cloud).to(dev), grid, b, coord_cols=4)
        sf.append(f)
        sc.append(c)
    labels = np.empty(B, dtype=object)
    for b in range(B):
        labels[b] = synth.synth_labels("Car", 6, seed=7000 + b)
    batch = (None, labels, sf, None, sc, None, None)
    steppers = {}
    for kind in ("atss", "simota"):
        torch.manual_seed(0)
        m = M.RPN3D("Car", target_assign=kind).to(dev).train()
        opt = ClipSGD(list(m.parameters()), 1e-3, 5.0)

        def step(m=m, opt=opt):          # RPN3D.train_step's separate-calls branch, for both kinds
            out = m(batch, dev)
            out[2].backward()
            opt.step()
            for p in m.parameters():
                p.grad = None
        steppers[kind] = step
    for step in steppers.values():
        for _ in range(5):
            step()
    torch.cuda.synchronize()
    ms = {k: [] for k in steppers}
    for _ in range(args.step_rounds):
        for kind, step in steppers.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(args.round_steps):
                step()
            e.record()
            torch.cuda.synchronize()
            ms[kind].append(s.elapsed_time(e) / args.round_steps)
    say(f"== RPN3D.train_step, separate calls, Car, B = {B}, 6 cars per frame, bf16: {args.step_rounds} alternated rounds of "
        f"{args.round_steps} steps; ms per step, median [min, max] ==")
    for kind, v in ms.items():
        say(f"target_assign {kind:8s} {statistics.median(v):9.3f} [{min(v):8.3f}, {max(v):8.3f}]")
    a_, o_ = statistics.median(ms["atss"]), statistics.median(ms["simota"])
    say(f"simota / atss: {o_:.3f} / {a_:.3f} = {o_ / a_:.3f}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
