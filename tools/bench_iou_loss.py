"""The rotated-IoU regression term alone — vn_rpn_iou_loss (csrc/iou_loss.hip): the three launches of one call
(normaliser partial sums, the pass over the (B, h, w) anchor sites that writes every element of d_delta, the one-workgroup
finish), and once without d_delta (the forward alone) — beside the reference loss pass (vn_rpn_loss_spec_fwd_bwd_rows with
bf16 rows, tools/bench_loss.py's launch), alternated inside one process, on two maps: the car step's (B = 2, 200 x 176:
70,400 sites) and the dense config's batch 4 (140,800 sites), each with about 60 positives per sample (what a KITTI frame
gives) and, as a stress case, 5 % positives.  Only positives do geometry: the first case is the latency of a few threads'
float64 chains beside the store of the 14 gradient channels, the second has a positive in nearly every wave.  The
positives' boxes overlap their targets (delta = target + uniform +-0.2, yaw +-0.5), so every one of them runs the clip and
the derivative.
Per arm and round: --round-launches calls back to back between two device events (us per call as the device saw them);
reported: the median over the rounds with min / max beside it.  No threshold is set on these numbers.
usage: python tools/bench_iou_loss.py [--rounds 20] [--round-launches 50] [--out FILE]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import torch
from voxelnet_amd import _lib
from voxelnet_amd import iou_loss as IL
from voxelnet_amd import model as M
from voxelnet_amd.targets import generate_anchors

dev = "cuda:0"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--round-launches", type=int, default=50)
ap.add_argument("--out")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_iou_loss.py needs cuda:0 (there is no CPU path to measure)")
if args.rounds < 5 or args.rounds * args.round_launches < 50:
    sys.exit("at least 5 rounds and 50 timed launches per arm")

lib = _lib.load()
st = _lib.raw_stream()
ABS = (1.5, 1.0, 3.0)
H, W = 200, 176
SHAPES = [("car B=2", 2), ("dense B=4", 4)]
DENSITIES = [("~60 / sample", 60.0 / (H * W * 2)), ("5 %", 0.05)]
TERMS = [("iou 3d", "iou", "3d", True), ("diou 3d", "diou", "3d", True), ("diou bev", "diou", "bev", True),
         ("iou 3d, forward only", "iou", "3d", False)]          # (the last: d_delta = NULL, the value without the derivative)
anchors = torch.from_numpy(generate_anchors("Car").reshape(-1, 7).copy()).to(dev)


def make(B, frac):
    g = torch.Generator().manual_seed(B)
    prob = torch.rand((B, 2, H, W), generator=g) * 0.98 + 0.01
    pos = (torch.rand((B, H, W, 2), generator=g) < frac).float()
    neg = (torch.rand((B, H, W, 2), generator=g) < 0.98).float() * (1 - pos)
    tgt = torch.rand((B, H, W, 14), generator=g) * 0.6 - 0.3
    noise = torch.rand((B, H, W, 14), generator=g) * 0.4 - 0.2
    noise[..., 6::7] = torch.rand((B, H, W, 2), generator=g) - 0.5
    delta = (tgt + noise).permute(0, 3, 1, 2).contiguous()
    ins = [t.to(dev).contiguous() for t in (prob, delta, pos, neg, tgt)]
    wsb, iwsb = lib.vn_rpn_loss_workspace_bytes(B, H, W), lib.vn_rpn_iou_loss_workspace_bytes(B, H, W)
    buf = {"ins": ins, "wsb": wsb, "ws": torch.zeros(wsb, dtype=torch.uint8, device=dev), "iwsb": iwsb,
           "iws": torch.zeros(iwsb, dtype=torch.uint8, device=dev), "dp": torch.empty_like(ins[0]), "dd": torch.empty_like(ins[1]),
           "idd": torch.empty_like(ins[1]), "rows": torch.empty((B * H * W, 16), dtype=torch.bfloat16, device=dev),
           "one": torch.ones(1, device=dev), "out2": torch.empty(2, device=dev), "n_pos": int(pos.sum())}
    _lib.call("vn_rpn_loss_norm", ins[2].data_ptr(), ins[3].data_ptr(), B, H, W, buf["ws"].data_ptr(), wsb, st)
    return buf


def checked(fn, a, name):
    def run():
        rc = fn(*a)
        if rc != 0:
            raise _lib.VoxelnetHipError(f"{name}: status {rc}")
    return run


def reference_launcher(buf, B):
    a = [t.data_ptr() for t in buf["ins"]] + [B, H, W, *ABS, buf["ws"].data_ptr(), buf["wsb"], buf["one"].data_ptr(),
                                              buf["dp"].data_ptr(), buf["dd"].data_ptr(), buf["rows"].data_ptr(), _lib.VN_BF16, 16, 0,
                                              st, ctypes.byref(M.loss_spec())]
    return checked(lib.vn_rpn_loss_spec_fwd_bwd_rows, a, "vn_rpn_loss_spec_fwd_bwd_rows")


def iou_launcher(buf, B, kind, metric, backward):
    _, delta, pos, _, tgt = buf["ins"]
    a = [delta.data_ptr(), pos.data_ptr(), tgt.data_ptr(), anchors.data_ptr(), B, H, W, IL.KINDS[kind], IL.METRICS[metric],
         buf["one"].data_ptr(), buf["iws"].data_ptr(), buf["iwsb"], buf["out2"].data_ptr(), buf["idd"].data_ptr() if backward else None, st]
    return checked(lib.vn_rpn_iou_loss, a, "vn_rpn_iou_loss")


arms = []          # (map, positives, arm, buffers, launcher)
for sname, B in SHAPES:
    for dname, frac in DENSITIES:
        buf = make(B, frac)
        arms.append((sname, dname, "reference loss pass", buf, reference_launcher(buf, B)))
        for tname, kind, metric, backward in TERMS:
            arms.append((sname, dname, tname, buf, iou_launcher(buf, B, kind, metric, backward)))
for *_, run in arms:                              # warm-up: code objects, the caches
    for _ in range(20):
        run()
torch.cuda.synchronize()
us = {a[:3]: [] for a in arms}
for _ in range(args.rounds):
    for sname, dname, aname, _, run in arms:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(args.round_launches):
            run()
        e.record()
        torch.cuda.synchronize()
        us[(sname, dname, aname)].append(s.elapsed_time(e) / args.round_launches * 1e3)

say(f"== rotated-IoU term (one vn_rpn_iou_loss call: 3 launches, d_delta written) beside the reference loss pass (1 launch), "
    f"{args.rounds} alternated rounds of {args.round_launches} calls per arm; median [min, max] over the rounds ==")
say(f"{'map':10s} {'positives':>14s} {'n_pos':>7s} {'arm':20s} {'us / call':>24s} {'vs loss pass':>13s}")
for sname, dname, aname, buf, _ in arms:
    v = us[(sname, dname, aname)]
    med = statistics.median(v)
    ratio = med / statistics.median(us[(sname, dname, "reference loss pass")])
    say(f"{sname:10s} {dname:>14s} {buf['n_pos']:7d} {aname:20s} {med:8.2f} [{min(v):6.2f}, {max(v):6.2f}] {ratio:12.2f}x")
    torch.cuda.synchronize()
    if aname != "reference loss pass" and not (torch.isfinite(buf["out2"]).all() and torch.isfinite(buf["idd"]).all()):
        sys.exit(f"{sname} {dname} {aname}: non-finite results")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
