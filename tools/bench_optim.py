"""The optimizer tail alone on the detector's real tensor set: RPN3D("Car"), 104 tensors, 6,809,392 elements, gradients in
the module's flat gradient buffer (what RPN3D.train_step leaves in .grad).  Four arms, alternated inside one process:
  clip_sgd      voxelnet_amd.optim.ClipSGD              (vn_clip_sgd, csrc/optim.hip: two launches)
  clip_adamw    voxelnet_amd.optim.ClipAdamW            (vn_clip_adamw, csrc/optim.hip: two launches)
  torch_foreach clip_grad_norm_ + torch.optim.AdamW(foreach=True)
  torch_fused   clip_grad_norm_ + torch.optim.AdamW(fused=True)
Per arm and round: ROUND updates back to back between two device events (us per update as the device saw them, host gaps
included when the host is the slower side), and a host clock around the same calls WITHOUT a synchronise (us of host
enqueue per update).  Reported: mean +- sd over the rounds, and the bytes/s of the counted-from-shapes traffic model —
32 B per element for AdamW (g read twice; p, m, v read and written), 16 B for SGD (g read twice, p read and written) — as a
share of the 6.29 TB/s copy rate measured on the MI355X.  Every arm has its own copy of the parameters; all
read the same gradients (torch's clip_grad_norm_ scales them in place at its first update, after which no arm clips).
No threshold is set on these numbers.
usage: python tools/bench_optim.py [--rounds 6] [--round-updates 50] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import torch
from voxelnet_amd import model as M
from voxelnet_amd.optim import ClipAdamW, ClipSGD, decay_param_groups

COPY_RATE = 6.29e12          # B/s, the project's measured device copy rate
dev = "cuda:0"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=6)
ap.add_argument("--round-updates", type=int, default=50)
ap.add_argument("--out")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_optim.py needs cuda:0 (there is no CPU path to measure)")
if args.rounds * args.round_updates < 200:
    sys.exit("at least 200 updates per arm")

torch.manual_seed(0)
model = M.RPN3D("Car").to(dev).train(True)
views = M._grad_views(model)                      # name -> view of the flat gradient buffer
named = model._named_params()
n_elems = sum(p.numel() for _, p in named)
assert len(named) == 104 and n_elems == 6809392
for n, _ in named:
    views[n].normal_(0.0, 1e-2)                   # total norm ~ 26: clipped at 5 until torch scales the buffer


def twin():
    """a second module with the same values whose parameters' .grad ARE the first one's gradient views"""
    m = M.RPN3D("Car").to(dev).train(True)
    m.load_state_dict(model.state_dict())
    for n, p in m.named_parameters():
        p.grad = views[n]
    return m


def arm_clip_sgd():
    opt = ClipSGD(list(twin().parameters()), 1e-4, 5.0)
    return opt.step, 16.0


def arm_clip_adamw():
    opt = ClipAdamW(decay_param_groups(twin(), 0.01), lr=1e-4, max_norm=5.0)
    return opt.step, 32.0


def arm_torch(**kw):
    m = twin()
    params = list(m.parameters())
    opt = torch.optim.AdamW(decay_param_groups(m, 0.01), lr=1e-4, **kw)

    def step():
        torch.nn.utils.clip_grad_norm_(params, 5.0)
        opt.step()
    return step, 32.0


ARMS = [("clip_sgd", arm_clip_sgd()), ("clip_adamw", arm_clip_adamw()), ("torch_foreach", arm_torch(foreach=True)),
        ("torch_fused", arm_torch(fused=True))]
for _, (fn, _) in ARMS:                           # warm-up: code objects, state, chunk tables, the allocator
    for _ in range(10):
        fn()
torch.cuda.synchronize()
dev_us = {name: [] for name, _ in ARMS}
host_us = {name: [] for name, _ in ARMS}
for _ in range(args.rounds):
    for name, (fn, _) in ARMS:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.record()
        for _ in range(args.round_updates):
            fn()
        e.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        dev_us[name].append(s.elapsed_time(e) / args.round_updates * 1e3)
        host_us[name].append((t1 - t0) / args.round_updates * 1e6)

say(f"== optimizer tail, RPN3D('Car'): {len(named)} tensors, {n_elems} elements, flat gradient buffer; {args.rounds} alternated "
    f"rounds of {args.round_updates} updates per arm; mean +- sd over the rounds ==")
say(f"{'arm':14s} {'us / update (device events)':>30s} {'us / update (host enqueue)':>30s} {'model bytes/s':>16s} {'of 6.29 TB/s':>13s}")
for name, (_, bpe) in ARMS:
    d, h = dev_us[name], host_us[name]
    rate = bpe * n_elems / (statistics.mean(d) * 1e-6)
    say(f"{name:14s} {statistics.mean(d):18.1f} +- {statistics.stdev(d):8.1f} {statistics.mean(h):18.1f} +- {statistics.stdev(h):8.1f} "
        f"{rate / 1e12:13.2f} TB {100.0 * rate / COPY_RATE:11.1f} %")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
