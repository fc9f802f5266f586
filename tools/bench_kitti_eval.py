"""What the image-plane scoring costs beside the scoring it extends (csrc/eval.hip):
`vn_boxes_to_image` + `vn_eval_match_image` against `vn_eval_match` on the same frames, in the same process — B = 2 and 64
frames, top_k = 20 detections, 12 and 128 ground truths per frame, four difficulties, 5 DontCare regions per frame, the
mean calibration.  Arms: the baseline launch, the new pair, and the pair's two kernels alone.

Method (tools/bench_loss.py's): every arm runs `--round-launches` times back to back between two device events, the arms
ALTERNATE over `--rounds` rounds; reported: the median over the rounds with min / max beside it, and the ratio to the
baseline's median.  No threshold is set on these numbers.  Expected: phase 1's clippings (one per pair, the same in both
matchers) dominate, so the pair should cost about one extra launch over vn_eval_match, not a multiple of it.
usage: python tools/bench_kitti_eval.py [--rounds 20] [--round-launches 50] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import numpy as np
import torch
from voxelnet_amd import _lib
from voxelnet_amd.evaluate import MIN_HEIGHT, _calib_rows

dev = "cuda:0"
TOP_K, N_DIFF, N_DC = 20, 4, 5
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--round-launches", type=int, default=50)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.rounds < 5 or args.rounds * args.round_launches < 50:
    sys.exit("at least 5 rounds and 50 timed launches per arm")


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def frame(rng, n_gt):
    """n_gt ground truths on a grid (disjoint, car-sized; tools/bench_eval.py's), TOP_K detections: jittered copies"""
    gt = np.array([[6.0 + 5.0 * (k % 13), -31.5 + 7.0 * (k // 13), -1.6, 1.5, 1.6, 4.0, 0.3 * ((k % 5) - 2)] for k in range(n_gt)])
    det = gt[rng.integers(0, n_gt, TOP_K)].copy()
    det[:, 0:2] += rng.normal(0, 0.25, (TOP_K, 2))
    det[:, 6] += rng.normal(0, 0.1, TOP_K)
    det[:, 3:6] *= rng.uniform(0.93, 1.07, (TOP_K, 3))
    return det.astype(np.float32), (0.96 + 0.04 * rng.random(TOP_K)).astype(np.float32), gt, rng.random((N_DIFF, n_gt)) < 0.3


def make(B, n_gt):
    rng = np.random.default_rng(B * 1000 + n_gt)
    fr = [frame(rng, n_gt) for _ in range(B)]
    t = {"det": up(np.stack([f[0] for f in fr])), "sc": up(np.stack([f[1] for f in fr])), "dc": up(np.full(B, TOP_K, dtype=np.int32)),
         "gt": up(np.stack([f[2] for f in fr])), "gc": up(np.full(B, n_gt, dtype=np.int32)),
         "fl": up(np.stack([f[3] for f in fr]).astype(np.uint8)),
         "cal": up(np.tile(_calib_rows(None)[0], (B, 1))), "hw": up(np.tile(np.array([375, 1242], dtype=np.int32), (B, 1))),
         "mh": up(np.array([MIN_HEIGHT[d] for d in ("all", "easy", "moderate", "hard")], dtype=np.float64)),
         "ga": up(rng.uniform(-3, 3, (B, n_gt))), "dcc": up(np.full(B, N_DC, dtype=np.int32))}
    x1, y1 = rng.uniform(0, 1100, (B, N_DC)), rng.uniform(120, 260, (B, N_DC))
    t["dcb"] = up(np.stack([x1, y1, x1 + rng.uniform(10, 120, (B, N_DC)), y1 + rng.uniform(10, 50, (B, N_DC))], axis=-1))
    t["rows"] = torch.empty((B, TOP_K, 12), dtype=torch.float64, device=dev)
    t["on"] = torch.empty((B, TOP_K), dtype=torch.uint8, device=dev)
    for k, m in (("st2", 2), ("st3", 3)):
        t[k] = torch.empty((B, m, N_DIFF, TOP_K), dtype=torch.int8, device=dev)
        t["mg" + k[2]] = torch.empty((B, m, N_DIFF, TOP_K), dtype=torch.int32, device=dev)
    t["sim"] = torch.empty((B, N_DIFF, TOP_K), dtype=torch.float64, device=dev)
    t["wsb"] = _lib.load().vn_eval_match_workspace_bytes(B, TOP_K, n_gt)
    t["ws"] = torch.empty(t["wsb"], dtype=torch.uint8, device=dev)
    return t


def launchers(t, B, n_gt):
    st = _lib.raw_stream()
    p = {k: v.data_ptr() for k, v in t.items() if torch.is_tensor(v)}

    def project():
        _lib.call("vn_boxes_to_image", p["det"], p["dc"], p["cal"], p["hw"], B, TOP_K, p["rows"], p["on"], st)

    def match_image():
        _lib.call("vn_eval_match_image", p["det"], p["sc"], p["dc"], p["gt"], p["gc"], p["fl"], p["rows"], p["on"], p["gtbb"], p["ga"],
                  p["dcb"], p["dcc"], p["mh"], B, TOP_K, n_gt, N_DC, N_DIFF, 0.7, 0.7, 0.7, p["st3"], p["mg3"], p["sim"], None,
                  p["ws"], t["wsb"], st)

    def baseline():
        _lib.call("vn_eval_match", p["det"], p["sc"], p["dc"], p["gt"], p["gc"], p["fl"], B, TOP_K, n_gt, N_DIFF, 0.7, 0.7, p["st2"],
                  p["mg2"], None, p["ws"], t["wsb"], st)

    def pair():
        project()
        match_image()

    # the ground truths' 2D boxes: their own projections (the same kernel, once, on the ground truths as detections)
    gtb = torch.zeros((B, n_gt, 4), dtype=torch.float64, device=dev)
    for g0 in range(0, n_gt, TOP_K):
        n = min(TOP_K, n_gt - g0)
        boxes = torch.zeros((B, TOP_K, 7), dtype=torch.float32, device=dev)
        boxes[:, :n] = t["gt"][:, g0:g0 + n].float()
        cnt = torch.full((B,), n, dtype=torch.int32, device=dev)
        _lib.call("vn_boxes_to_image", boxes.data_ptr(), cnt.data_ptr(), p["cal"], p["hw"], B, TOP_K, p["rows"], p["on"], st)
        gtb[:, g0:g0 + n] = t["rows"][:, :n, 1:5]
    t["gtbb"] = gtb
    p["gtbb"] = gtb.data_ptr()
    return [("vn_eval_match", baseline), ("pair", pair), ("vn_boxes_to_image", project), ("vn_eval_match_image", match_image)]


arms = []
for n_gt in (12, 128):
    for B in (2, 64):
        t = make(B, n_gt)
        for name, run in launchers(t, B, n_gt):
            arms.append((f"B {B:2d} x {n_gt:3d} gt", name, t, run))
for *_, run in arms:                              # warm-up: code objects, the caches
    for _ in range(20):
        run()
torch.cuda.synchronize()
us = {(s, o): [] for s, o, *_ in arms}
for _ in range(args.rounds):
    for sname, oname, _, run in arms:
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(args.round_launches):
            run()
        e.record()
        torch.cuda.synchronize()
        us[(sname, oname)].append(s.elapsed_time(e) / args.round_launches * 1e3)

say(f"== image-plane scoring vs vn_eval_match: top_k {TOP_K}, {N_DIFF} difficulties, {N_DC} DontCare regions; {args.rounds} alternated "
    f"rounds of {args.round_launches} calls per arm; us per call, median [min, max] over the rounds ==")
say(f"{'frames':16s} {'arm':22s} {'us / call':>26s} {'vs vn_eval_match':>17s}")
for sname, oname, t, _ in arms:
    v = us[(sname, oname)]
    med = statistics.median(v)
    say(f"{sname:16s} {oname:22s} {med:8.2f} [{min(v):7.2f}, {max(v):7.2f}] {med / statistics.median(us[(sname, 'vn_eval_match')]):16.2f}x")
    if oname == "pair":          # the launches ran: look at their outputs once
        on = t["on"].bool()
        if not (on.any() and (t["st3"] != 99).all() and torch.isfinite(t["sim"]).all() and torch.isfinite(t["rows"]).all()):
            sys.exit(f"{sname}: implausible results")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
