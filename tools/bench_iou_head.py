"""Time the IoU-aware confidence head's passes, alternated inside one process.

1. Kernels, on the concatenation of the full Car grid (200 x 176 sites, 768 bf16 channels), B = 2 ("car") and B = 4 ("dense"):
     split forward              two vn_dir_head_fwd calls, one per head, back to back
     fused forward              one vn_site_heads_fwd call with n_out = 4
   each with the rows read from ONE buffer (108 / 216 MB: what the Infinity Cache can keep) and "cold", from a ring of
   buffers larger than the Infinity Cache together, one per call (the regimes of tools/bench_dir_head.py);
     vn_rpn_iou_head_loss       with the gradient and the target map, car map, the positives of 8 and of 128 boxes per frame
     vn_rpn_dir_loss            the same maps: the yardstick from the same run
     vn_iou_rectify_probs       the car map
2. --steps N > 0: RPN3D(iou_head=True).train_step against RPN3D(native_executor=False).train_step on the car config (both
   through the per-layer orchestration, the path the head runs on), and both heads on, alternated rounds of N steps.
Method of tools/bench_assign.py: per arm and round --round-launches calls back to back between two device events, the arms
alternated round by round; reported: median [min, max] over the rounds.  No threshold is set on these numbers.
usage: python tools/bench_iou_head.py [--rounds 20] [--round-launches 50] [--steps 0] [--out FILE]"""
import argparse
import math
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
from voxelnet_amd.voxelize import voxelize_device

dev = "cuda:0"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--round-launches", type=int, default=50)
ap.add_argument("--steps", type=int, default=0)
ap.add_argument("--step-rounds", type=int, default=5)
ap.add_argument("--out")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_iou_head.py needs cuda:0 (there is no CPU path to measure)")
if args.rounds < 5 or args.rounds * args.round_launches < 50:
    sys.exit("at least 5 rounds and 50 timed launches per arm")
lib = _lib.load()
st = _lib.raw_stream()
H, W, C = 200, 176, 768
S = H * W
IC_BYTES = 256 << 20
rng = np.random.default_rng(3)
anchors = torch.from_numpy(np.ascontiguousarray(T.generate_anchors("Car").reshape(-1, 7))).to(dev)
w4 = torch.from_numpy((rng.standard_normal((4, C)) * 0.05).astype(np.float32)).to(dev)
b4 = torch.zeros(4, dtype=torch.float32, device=dev)
arms = []


def forward_arms(tag, B):
    M_ = B * S
    nbytes = M_ * C * 2
    ring = [torch.randn((M_, C), device=dev).to(torch.bfloat16) for _ in range(IC_BYTES // nbytes + 2)]
    two = [torch.empty((B, 2, S), dtype=torch.float32, device=dev) for _ in range(2)]
    four = torch.empty((B, 4, S), dtype=torch.float32, device=dev)
    turn = {"split": 0, "fused": 0}

    def split(rows):
        for k in range(2):
            _lib.call("vn_dir_head_fwd", rows.data_ptr(), _lib.VN_BF16, C, w4[2 * k:].data_ptr(), b4[2 * k:].data_ptr(), B, S,
                      two[k].data_ptr(), st)

    def fused(rows):
        _lib.call("vn_site_heads_fwd", rows.data_ptr(), _lib.VN_BF16, C, w4.data_ptr(), b4.data_ptr(), 4, B, S, four.data_ptr(), st)

    def cold(fn, key):
        def run():
            turn[key] = (turn[key] + 1) % len(ring)
            fn(ring[turn[key]])
        return run
    note = f"{tag} B={B}, {nbytes / 1e6:.0f} MB"
    arms.append(("split forward (2 calls)", note, lambda: split(ring[0]), nbytes))
    arms.append(("fused forward", note, lambda: fused(ring[0]), nbytes))
    arms.append(("split forward cold", f"{note} x {len(ring)}", cold(split, "split"), nbytes))
    arms.append(("fused forward cold", f"{note} x {len(ring)}", cold(fused, "fused"), nbytes))
    split(ring[0])
    fused(ring[0])
    torch.cuda.synchronize()
    assert torch.equal(four[:, 0:2], two[0]) and torch.equal(four[:, 2:4], two[1]), "the fused forward is not the split one"
    return ring


def car_targets(G, B=2):
    cfg = T.CLASS_CFG["Car"]
    gen = T.TargetGenerator("Car", dev, assign="rotated")
    frames = []
    for b in range(B):
        r = np.random.default_rng(10 * G + b)
        frames.append(np.stack([r.uniform(4, 66, G), r.uniform(-36, 36, G), cfg["z"] + r.uniform(-0.2, 0.2, G),
                                cfg["h"] * r.uniform(0.9, 1.1, G), cfg["w"] * r.uniform(0.9, 1.1, G), cfg["l"] * r.uniform(0.9, 1.1, G),
                                r.uniform(-math.pi, math.pi, G)], axis=1))
    return gen.from_boxes(frames)


keep = [forward_arms("car", 2)]
B = 2
logits2 = torch.randn((B, 2, S), device=dev)
probs2 = torch.rand((B, 2, S), device=dev)
rect = torch.empty_like(probs2)
nb_loss = lib.vn_rpn_iou_head_loss_workspace_bytes(B, H, W)
ws_loss = torch.empty(nb_loss, dtype=torch.uint8, device=dev)
out2 = torch.empty(2, dtype=torch.float32, device=dev)
d_logits = torch.empty_like(logits2)
t_map = torch.empty_like(logits2)
for G in (8, 128):
    pos, neg, tgt = car_targets(G)
    # regression maps near their targets at the positives (IoU > 0: the full geometry runs), noise elsewhere
    delta = (tgt + 0.05 * torch.randn_like(tgt)).permute(0, 3, 1, 2).contiguous()
    keep += [pos, neg, tgt, delta]

    def head_loss(p=pos, t=tgt, d=delta):
        _lib.call("vn_rpn_iou_head_loss", logits2.data_ptr(), d.data_ptr(), p.data_ptr(), t.data_ptr(), anchors.data_ptr(), B, H, W,
                  _lib.VN_IOU_3D, ws_loss.data_ptr(), nb_loss, out2.data_ptr(), d_logits.data_ptr(), t_map.data_ptr(), st)

    def dir_loss(p=pos, t=tgt):
        _lib.call("vn_rpn_dir_loss", logits2.data_ptr(), p.data_ptr(), t.data_ptr(), anchors.data_ptr(), B, H, W, math.pi / 4,
                  ws_loss.data_ptr(), nb_loss, out2.data_ptr(), d_logits.data_ptr(), st)
    head_loss()
    torch.cuda.synchronize()
    note = f"car B=2, {G} boxes: {int((pos != 0).sum())} positives, mean target {float(t_map.sum() / max(1, int((pos != 0).sum()))):.3f}"
    arms.append(("vn_rpn_iou_head_loss", note, head_loss, None))
    arms.append(("vn_rpn_dir_loss", f"car B=2, {G} boxes", dir_loss, None))
arms.append(("vn_iou_rectify_probs", f"car B=2, {probs2.numel()} anchors", lambda: _lib.call(
    "vn_iou_rectify_probs", probs2.data_ptr(), logits2.data_ptr(), probs2.numel(), 0.5, rect.data_ptr(), st), None))
keep.append(forward_arms("dense", 4))

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
say(f"== IoU-aware head (full Car grid, {S} sites per frame): {args.rounds} alternated rounds of {args.round_launches} calls per arm; "
    f"us per call, median [min, max] over the rounds; GB/s of row bytes (read once) at the median ==")
for a, b, _, nbytes in arms:
    v = us[(a, b)]
    bw = f"{nbytes / statistics.median(v) / 1e3:8.0f} GB/s" if nbytes else ""
    say(f"{a:24s} {b:58s} {statistics.median(v):9.2f} [{min(v):8.2f}, {max(v):8.2f}] {bw}")
del keep
torch.cuda.empty_cache()

if args.steps > 0:
    from voxelnet_amd.optim import ClipSGD
    M.set_precision("bf16")
    grid = grid_config("Car")
    feats, coords = [], []
    for b, cloud in enumerate(synth.workload_frames(1, batch=2)):
        f, c, _ = voxelize_device(torch.from_numpy(cloud).to(dev), grid, b, coord_cols=4)
        feats.append(f)
        coords.append(c)
    labels = [synth.synth_labels("Car", 6, seed=7000 + b) for b in range(2)]
    batch = (None, labels, feats, None, coords, None, None)
    models = {}
    for name, kw in (("per-layer, no head", {}), ("per-layer, iou_head", {"iou_head": True}),
                     ("per-layer, dir_head", {"dir_head": True}), ("per-layer, dir + iou", {"dir_head": True, "iou_head": True})):
        torch.manual_seed(1)
        m = M.RPN3D("Car", cls_loss="focal", yaw_loss="sin", target_assign="rotated", **kw).to(dev).train()
        m.native_executor = False
        models[name] = (m, ClipSGD(list(m.parameters()), 0.01, 5.0))
    ms = {k: [] for k in models}
    for r in range(args.step_rounds + 1):
        for name, (m, opt) in models.items():
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.steps):
                m.train_step(batch, dev, opt)
                opt.zero_grad(set_to_none=True)
            e.record()
            torch.cuda.synchronize()
            if r:                                      # (round 0 warms up)
                ms[name].append(s.elapsed_time(e) / args.steps)
    say(f"== train_step on the car config, bf16, focal + sine, rotated assignment: {args.step_rounds} alternated rounds of {args.steps} "
        f"steps; ms per step, median [min, max] ==")
    for name, v in ms.items():
        say(f"{name:24s} {statistics.median(v):9.2f} [{min(v):8.2f}, {max(v):8.2f}]")
    del models
    torch.cuda.empty_cache()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
