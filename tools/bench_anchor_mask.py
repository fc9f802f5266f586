"""Time the anchor mask, alternated inside one process, on bench.py's synthetic clouds.

1. The library calls on the full Car grid (70,400 anchors per frame), for the car config (B = 2) and the dense config
   (B = 4): us per call (every launch of the call: vn_anchor_mask's memset + five kernels) for
     mask            vn_anchor_mask, mask only
     mask + edit     vn_anchor_mask with pos / neg edited in place (what RPN3D(anchor_area_threshold=) runs per step)
     probs flat/site vn_anchor_mask_probs (what the decode adds per batch)
     targets         vn_rpn_targets with 8 boxes per frame, from the same process: the yardstick — the mask runs beside it on
                     the targets stream
   and the share of anchors kept at thresholds 0 and 1 on those clouds.
2. RPN3D(anchor_area_threshold=1).train_step against the default train_step (car config, bf16, ClipSGD): ms per step.
3. RPN3D.evaluate with and without the mask on the car frames (predict.TRAINED_DECODE): ms per batch, the anchors at or above
   score_thres and the candidates that enter the NMS (an untrained model's maps: the counts say what the mask removes, not
   what a trained model would score).
Method of tools/bench_assign.py: per arm and round --round-launches calls back to back between two device events, the arms
alternated round by round; reported: median [min, max] over the rounds.  No threshold is set on these numbers.
usage: python tools/bench_anchor_mask.py [--rounds 20] [--round-launches 50] [--step-rounds 10] [--steps 5] [--out FILE]"""
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
from voxelnet_amd.anchor_mask import AnchorMasker
from voxelnet_amd.config import GRADIENT_CLIP, LR, grid_config
from voxelnet_amd.optim import ClipSGD
from voxelnet_amd.predict import TRAINED_DECODE, BoxDecoder
from voxelnet_amd.voxelize import voxelize_device

dev = "cuda:0"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--round-launches", type=int, default=50)
ap.add_argument("--step-rounds", type=int, default=10)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--out")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_anchor_mask.py needs cuda:0 (there is no CPU path to measure)")
if args.rounds < 5 or args.rounds * args.round_launches < 50 or args.step_rounds < 5:
    sys.exit("at least 5 rounds and 50 timed launches per arm")
lib = _lib.load()
st = _lib.raw_stream()
cfg = T.CLASS_CFG["Car"]
WORKLOADS = {"car": (2, 2, 35), "dense": (5, 4, 64)}          # bench.py CONFIGS: synth workload id, batch, T


def timed(arms, rounds, launches):
    for _, run in arms:                              # warm-up: code objects, the caches
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    t = {name: [] for name, _ in arms}
    for _ in range(rounds):
        for name, run in arms:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(launches):
                run()
            e.record()
            torch.cuda.synchronize()
            t[name].append(s.elapsed_time(e) / launches)
    return t


def voxels(name):
    wid, B, Tn = WORKLOADS[name]
    grid = grid_config("Car", T=Tn)
    feats, coords = [], []
    for b, cloud in enumerate(synth.workload_frames(wid, batch=B)):
        f, c, _ = voxelize_device(torch.from_numpy(cloud).to(dev), grid, b, coord_cols=4)
        feats.append(f)
        coords.append(c)
    return grid, B, feats, coords


# ---- 1. the library calls
keep_alive, arms, shares = [], [], []
for name in WORKLOADS:
    grid, B, _, coords = voxels(name)
    coord = torch.cat(coords).contiguous()
    mk = AnchorMasker("Car", dev, threshold=1, grid=grid)
    N, K = mk.n_anchors, coord.shape[0]
    nb = lib.vn_anchor_mask_workspace_bytes(B, grid.H, grid.W, N)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    mask = torch.empty((B, N), dtype=torch.uint8, device=dev)
    pos, neg = (torch.ones((B, N), dtype=torch.float32, device=dev) for _ in range(2))
    probs = torch.rand((B, N), dtype=torch.float32, device=dev)
    out = torch.empty_like(probs)

    def call_mask(edit, coord=coord, K=K, B=B, grid=grid, mk=mk, N=N, mask=mask, pos=pos, neg=neg, ws=ws, nb=nb):
        _lib.call("vn_anchor_mask", coord.data_ptr(), K, B, grid.H, grid.W, mk._rects_dev.data_ptr(), N, 1, mask.data_ptr(), None,
                  pos.data_ptr() if edit else None, neg.data_ptr() if edit else None, ws.data_ptr(), nb, st)

    def call_probs(layout, probs=probs, mask=mask, B=B, N=N, out=out):
        _lib.call("vn_anchor_mask_probs", probs.data_ptr(), mask.data_ptr(), B, N, layout, out.data_ptr(), st)

    G = 8
    rng = np.random.default_rng(80)
    frames = [np.stack([rng.uniform(4, 66, G), rng.uniform(-36, 36, G), np.full(G, cfg["z"]), np.full(G, cfg["h"]), np.full(G, cfg["w"]),
                        np.full(G, cfg["l"]), rng.uniform(-1.5, 1.5, G)], axis=1) for _ in range(B)]
    gt = torch.from_numpy(np.stack(frames)).to(dev)
    g2 = torch.from_numpy(np.stack([T.gt_standup_boxes(f) for f in frames])).to(dev)
    cnt = torch.full((B,), G, dtype=torch.int32, device=dev)
    anchors = torch.from_numpy(np.ascontiguousarray(mk.anchors.reshape(-1, 7))).to(dev)
    tp, tn = (torch.empty((B, N), dtype=torch.float32, device=dev) for _ in range(2))
    tt = torch.empty((B, N, 7), dtype=torch.float32, device=dev)
    tb = lib.vn_rpn_targets_workspace_bytes(B, N, G)
    tws = torch.empty(tb, dtype=torch.uint8, device=dev)
    ta = (anchors.data_ptr(), N, gt.data_ptr(), g2.data_ptr(), cnt.data_ptr(), B, G, cfg["pos_iou"], cfg["neg_iou"], cfg["h"],
          tp.data_ptr(), tn.data_ptr(), tt.data_ptr(), tws.data_ptr(), tb, st)
    keep_alive += [coord, mk, ws, mask, pos, neg, probs, out, gt, g2, cnt, anchors, tp, tn, tt, tws]
    tag = f"{name} B={B} K={K}"
    arms += [(f"{tag}: mask", lambda f=call_mask: f(False)), (f"{tag}: mask + edit", lambda f=call_mask: f(True)),
             (f"{tag}: probs flat", lambda f=call_probs: f(_lib.VN_DETECT_FLAT)), (f"{tag}: probs site", lambda f=call_probs: f(_lib.VN_DETECT_SITE)),
             (f"{tag}: vn_rpn_targets, {G} boxes", lambda a=ta: _lib.call("vn_rpn_targets", *a))]
    for thr in (0, 1):
        kept = AnchorMasker("Car", dev, threshold=thr, grid=grid).mask(coord, B)
        shares.append(f"{tag}: threshold {thr}: {float(kept.float().mean()):.4f} of the {B} x {N} anchors kept")

us = timed(arms, args.rounds, args.round_launches)
say(f"== anchor mask, full Car grid: {args.rounds} alternated rounds of {args.round_launches} calls per arm; us per call, median "
    f"[min, max] over the rounds ==")
for name, _ in arms:
    v = [x * 1e3 for x in us[name]]
    say(f"{name:48s} {statistics.median(v):9.2f} [{min(v):8.2f}, {max(v):8.2f}]")
for s in shares:
    say(s)

# ---- 2. the train step, 3. evaluate (car config, bf16)
M.set_precision("bf16")
grid, B, feats, coords = voxels("car")
labels = [synth.synth_labels("Car", 6, seed=7000 + b) for b in range(B)]
batch = ([f"{b:06d}" for b in range(B)], labels, feats, None, coords, None, None)
models = {}
for name, kw in (("default", {}), ("anchor_area_threshold=1", dict(anchor_area_threshold=1))):
    torch.manual_seed(0)
    m = M.RPN3D("Car", **kw).to(dev).train()
    models[name] = (m, ClipSGD(list(m.parameters()), LR, GRADIENT_CLIP))


def step(name):
    m, opt = models[name]
    opt.zero_grad(set_to_none=True)
    m.train_step(batch, dev, opt)


ms = timed([(n, lambda n=n: step(n)) for n in models], args.step_rounds, args.steps)
say(f"== RPN3D.train_step (car, bf16, B = {B}): {args.step_rounds} alternated rounds of {args.steps} steps; ms per step ==")
for name in models:
    v = ms[name]
    say(f"{name:48s} {statistics.median(v):9.3f} [{min(v):8.3f}, {max(v):8.3f}]")

dec = BoxDecoder("Car", dev)


def evaluate(name):
    models[name][0].evaluate([batch], dev, decoder=dec, decode=TRAINED_DECODE)


ms = timed([(n, lambda n=n: evaluate(n)) for n in models], args.step_rounds, args.steps)
say(f"== RPN3D.evaluate (car, bf16, B = {B}, predict.TRAINED_DECODE): ms per batch ==")
for name in models:
    v = ms[name]
    say(f"{name:48s} {statistics.median(v):9.3f} [{min(v):8.3f}, {max(v):8.3f}]")
thres, pre = TRAINED_DECODE["score_thres"], TRAINED_DECODE["pre_nms_top_k"]
for name, (m, _) in models.items():
    m.eval()
    with torch.no_grad():
        prob, delta = m.detect(feats, coords)
    mask = m._decode_mask(dec, coords, dev) if m.anchor_area_threshold is not None else None
    cc = dec.candidates_device(prob, delta, thres, pre, layout="site", anchor_mask=mask)[3]
    p = prob if mask is None else dec._masked(prob, mask, thres, "site", "bench")
    say(f"{name}: anchors with score >= {thres}: {(p >= thres).sum(dim=(1, 2, 3)).tolist()}; candidates entering the NMS (cap {pre}): "
        f"{cc.tolist()}")
    m.train()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
