"""The optimizer tail with a weight average (csrc/optim.hip, voxelnet_amd/ema.py) on the detector's
104 parameter tensors (6,809,392 elements) and 50 running-statistics buffers, for both update rules, four arms:
  0. no average                      ClipSGD / ClipAdamW .step()                      (the tail as it was)
  1. fused                           .step() with a ModelEMA attached                 (vn_clip_*_ema + vn_ema_update on the buffers)
  2. plain tail + vn_ema_update      .step(), then ModelEMA.update()                  (one launch over all 154 tensors)
  3. plain tail + torch              .step(), then torch._foreach_lerp_ over the 154 tensors
Gradients are views of one flat buffer, as RPN3D leaves them (the chunk tables are built once).  The arms are interleaved,
>= 12 rounds; a round of an arm is a train of 50 tails between two device events (device time per tail) and the same
train's wall time (what the host adds).  Mean +- sd per arm and the paired differences against arm 0.
With --ab DIR/TAG every round of every arm is also written as DIR/TAG_<rule>_{dev,wall}_<arm>_<round>.json ({"value":
microseconds}) — the files `tools/ab_stats.py TAG_sgd_dev DIR` reads (its verdict column is worded for a throughput: for
these microsecond values a NEGATIVE paired difference is the faster arm).
usage: python tools/bench_ema.py [--rounds N] [--out FILE] [--ab DIR/TAG]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import numpy as np
import torch
from voxelnet_amd import model as M
from voxelnet_amd.ema import ModelEMA
from voxelnet_amd.optim import ClipAdamW, ClipSGD, decay_param_groups

dev = "cuda:0"
HBM = 6.29e12          # B/s, measured float4 copy on the MI355X
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 12
AB = sys.argv[sys.argv.index("--ab") + 1] if "--ab" in sys.argv else None
TRAIN = 50
ARMS = ["no average", "fused", "tail + vn_ema_update", "tail + torch._foreach_lerp_"]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def build(rule, arm):
    """one detector's tensors, an optimizer and the arm's tail as a callable"""
    torch.manual_seed(5)
    model = M.RPN3D("Car").to(dev)
    params = list(model.parameters())
    flat = torch.randn(sum(p.numel() for p in params), device=dev) * 1e-3
    off = 0
    for p in params:
        p.grad = flat[off:off + p.numel()].view_as(p)
        off += p.numel()
    if rule == "sgd":
        opt = ClipSGD(params, lr=1e-6, max_norm=5.0)
    else:
        opt = ClipAdamW(decay_param_groups(model, 0.01), lr=1e-6, max_norm=5.0)
    if arm == 0:
        return opt.step
    if arm == 1:
        ModelEMA(model, opt, decay=0.999, warmup=None)
        return opt.step
    if arm == 2:
        avg = ModelEMA(model, decay=0.999, warmup=None)

        def tail():
            opt.step()
            avg.update()
        return tail
    live = [t.detach() for t in model.state_dict().values() if t.is_floating_point()]
    shadow = [t.clone() for t in live]

    def tail():
        opt.step()
        torch._foreach_lerp_(shadow, live, 1.0 - 0.999)
    return tail


def one_round(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    s.record()
    for _ in range(TRAIN):
        fn()
    e.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / TRAIN * 1e6
    return s.elapsed_time(e) / TRAIN * 1e3, wall          # us, us


N = 6809392
say(f"== optimizer tail on the detector's tensors ({N} parameter elements), us per tail in a train of {TRAIN}, {ROUNDS} interleaved rounds ==")
for rule, base_bytes in (("sgd", 16.0), ("adamw", 32.0)):
    tails = [build(rule, a) for a in range(len(ARMS))]
    devt = [[] for _ in ARMS]
    wall = [[] for _ in ARMS]
    for rnd in range(ROUNDS):
        for k, fn in enumerate(tails):
            d, w = one_round(fn)
            devt[k].append(d)
            wall[k].append(w)
            if AB:
                os.makedirs(os.path.dirname(os.path.abspath(AB)), exist_ok=True)
                for what, v in (("dev", d), ("wall", w)):
                    with open(f"{AB}_{rule}_{what}_{k}_{rnd}.json", "w") as f:
                        f.write(json.dumps({"value": v, "arm": ARMS[k]}) + "\n")
    if AB:
        for what in ("dev", "wall"):
            open(f"{AB}_{rule}_{what}_arms.txt", "w").write("\n".join(ARMS) + "\n")
    say(f"-- {rule}: both launches move {base_bytes:.0f} B per element ({base_bytes * N / HBM * 1e6:.1f} us at 6.29 TB/s); the fused "
        f"average adds 8 B ({8.0 * N / HBM * 1e6:.1f} us), a pass of its own 12 B ({12.0 * N / HBM * 1e6:.1f} us) and a launch --")
    for k, a in enumerate(ARMS):
        d, w = np.array(devt[k]), np.array(wall[k])
        say(f"{k} {a:28s}: device {d.mean():8.2f} +- {d.std(ddof=1):5.2f} us   wall {w.mean():8.2f} +- {w.std(ddof=1):5.2f} us")
    for k in range(1, len(ARMS)):
        dd, dw = np.array(devt[k]) - np.array(devt[0]), np.array(wall[k]) - np.array(wall[0])
        say(f"paired difference {k} - 0 ({ROUNDS} rounds, mean +- s.e.): device {dd.mean():+8.2f} +- {dd.std(ddof=1) / np.sqrt(len(dd)):5.2f} us"
            f"   wall {dw.mean():+8.2f} +- {dw.std(ddof=1) / np.sqrt(len(dw)):5.2f} us")
    del tails
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")
