"""The loss pass of the train step alone — vn_rpn_loss_spec_fwd_bwd_rows with bf16 rows: ONE launch over the (B, h, w)
anchor sites that writes the forward partial sums, d_prob, d_delta and the heads' (B*S, 16) gradient rows (what vn_net_step
puts between the network's forward and backward) — for two objectives, alternated inside one process:
  reference     the zeroed vnLossSpec: balanced cross-entropy + smooth-L1 (the instantiation the benchmark's step runs)
  focal+sin     cls_kind = VN_LOSS_FOCAL (focal_alpha 0.25, --gamma, default 2) with yaw_sin = 1
on two maps: the car step's (B = 2, 200 x 176: 70,400 sites) and the dense config's batch 4 (140,800 sites).
Per arm and round: --round-launches launches back to back between two device events (us per launch as the device saw
them: the kernel plus the boundary to its successor; the host enqueues faster than that).  Reported: the median over the
rounds, min / max beside it, and the bytes/s of the counted-from-shapes traffic — per site 34 fp32 read (prob 2, delta 14,
pos 2, neg 2, targets 14), 16 fp32 written (d_prob 2, d_delta 14) and 16 bf16 rows written: 232 B — as a share of the
8.0 TB/s HBM3E peak and of the 6.29 TB/s copy rate measured on the MI355X.  The same buffers are read by every launch and
are small enough (16 / 33 MB) to stay in the 256 MB Infinity Cache, so the share says how far the launch is from the HBM
bound it would have in the step, where the maps arrive from the heads' kernel; it is not a measurement of HBM traffic.
No threshold is set on these numbers.
usage: python tools/bench_loss.py [--rounds 20] [--round-launches 50] [--gamma 2.0] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import torch
from voxelnet_amd import _lib
from voxelnet_amd import model as M

HBM_PEAK, COPY_RATE = 8.0e12, 6.29e12          # B/s
BYTES_PER_SITE = 34 * 4 + 16 * 4 + 16 * 2
dev = "cuda:0"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--round-launches", type=int, default=50)
ap.add_argument("--gamma", type=float, default=2.0)
ap.add_argument("--out")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_loss.py needs cuda:0 (there is no CPU path to measure)")
if args.rounds < 5 or args.rounds * args.round_launches < 50:
    sys.exit("at least 5 rounds and 50 timed launches per arm")

lib = _lib.load()
st = _lib.raw_stream()
ABS = (1.5, 1.0, 3.0)
SPECS = [("reference", M.loss_spec()), ("focal+sin", M.loss_spec("focal", 0.25, args.gamma, "sin"))]
SHAPES = [("car B=2", 2, 200, 176), ("dense B=4", 4, 200, 176)]


def make(B, H, W):
    g = torch.Generator().manual_seed(B)
    prob = torch.rand((B, 2, H, W), generator=g) * 0.98 + 0.01
    delta = torch.randn((B, 14, H, W), generator=g) * 0.2
    pos = (torch.rand((B, H, W, 2), generator=g) < 0.002).float()          # a few dozen positives per frame
    neg = (torch.rand((B, H, W, 2), generator=g) < 0.98).float() * (1 - pos)
    tgt = torch.randn((B, H, W, 14), generator=g) * 0.2
    ins = [t.to(dev).contiguous() for t in (prob, delta, pos, neg, tgt)]
    wsb = lib.vn_rpn_loss_workspace_bytes(B, H, W)
    buf = {"ins": ins, "wsb": wsb, "ws": torch.zeros(wsb, dtype=torch.uint8, device=dev),
           "dp": torch.empty_like(ins[0]), "dd": torch.empty_like(ins[1]),
           "rows": torch.empty((B * H * W, 16), dtype=torch.bfloat16, device=dev), "one": torch.ones(1, device=dev),
           "out": torch.empty(5, device=dev)}
    _lib.call("vn_rpn_loss_norm", ins[2].data_ptr(), ins[3].data_ptr(), B, H, W, buf["ws"].data_ptr(), wsb, st)
    return buf


def launcher(buf, B, H, W, spec):
    a = [t.data_ptr() for t in buf["ins"]] + [B, H, W, *ABS, buf["ws"].data_ptr(), buf["wsb"], buf["one"].data_ptr(),
                                              buf["dp"].data_ptr(), buf["dd"].data_ptr(), buf["rows"].data_ptr(), _lib.VN_BF16, 16, 0,
                                              st, ctypes.byref(spec)]
    fn = lib.vn_rpn_loss_spec_fwd_bwd_rows

    def run():
        rc = fn(*a)
        if rc != 0:
            raise _lib.VoxelnetHipError(f"vn_rpn_loss_spec_fwd_bwd_rows: status {rc}")
    return run


arms = []
for sname, B, H, W in SHAPES:
    buf = make(B, H, W)
    for oname, spec in SPECS:
        arms.append((sname, oname, B * H * W, buf, launcher(buf, B, H, W, spec)))
for *_, run in arms:                              # warm-up: code objects, the caches
    for _ in range(20):
        run()
torch.cuda.synchronize()
us = {(s, o): [] for s, o, *_ in arms}
for _ in range(args.rounds):
    for sname, oname, _, _, run in arms:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(args.round_launches):
            run()
        e.record()
        torch.cuda.synchronize()
        us[(sname, oname)].append(s.elapsed_time(e) / args.round_launches * 1e3)

say(f"== loss pass (sums + gradients + bf16 head rows in one launch), {args.rounds} alternated rounds of {args.round_launches} "
    f"launches per arm, focal gamma {args.gamma:g}; median [min, max] over the rounds; {BYTES_PER_SITE} B per site ==")
say(f"{'map':10s} {'objective':10s} {'sites':>8s} {'us / launch':>24s} {'model bytes/s':>14s} {'of 8.0 TB/s':>12s} {'of 6.29 TB/s':>13s} "
    f"{'vs reference':>13s}")
for sname, oname, sites, buf, _ in arms:
    v = us[(sname, oname)]
    med = statistics.median(v)
    rate = BYTES_PER_SITE * sites / (med * 1e-6)
    ratio = med / statistics.median(us[(sname, "reference")])
    say(f"{sname:10s} {oname:10s} {sites:8d} {med:8.2f} [{min(v):6.2f}, {max(v):6.2f}] {rate / 1e12:11.2f} TB {100 * rate / HBM_PEAK:10.1f} % "
        f"{100 * rate / COPY_RATE:11.1f} % {ratio:12.2f}x")
    # the launches ran: finish the sums and look at them once
    B = buf["ins"][0].shape[0]
    _lib.call("vn_rpn_loss_finalize", buf["ws"].data_ptr(), buf["wsb"], B, 200, 176, ABS[0], ABS[1], buf["out"].data_ptr(), st)
    torch.cuda.synchronize()
    if not (torch.isfinite(buf["out"]).all() and torch.isfinite(buf["dp"]).all() and torch.isfinite(buf["rows"].float()).all()):
        sys.exit(f"{sname} {oname}: non-finite results")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
