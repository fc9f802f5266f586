"""Time the direction-classifier head's passes, alternated inside one process.

1. Kernels, on the concatenation of the full Car grid (200 x 176 sites, 768 bf16 channels), B = 2 ("car") and B = 4 ("dense"):
     vn_dir_head_fwd            the rows read back to back from one buffer (108 / 216 MB: what the Infinity Cache can keep),
     vn_dir_head_fwd cold       and from a ring of buffers larger than the Infinity Cache together, one per launch
     vn_heads_fwd (+ cold)      the two heads over the same rows: the yardstick from the same run
     vn_dir_head_bwd            car map, the positives of 8 and of 128 boxes per frame (rotated assignment)
     vn_rpn_dir_loss            with the gradient
2. --steps N > 0: RPN3D(dir_head=True).train_step against RPN3D(native_executor=False).train_step on the car config (both
   through the per-layer orchestration, the path the head runs on), alternated rounds of N steps, ms per step.
3. --fit N > 0: N ClipAdamW steps (lr 1e-3, focal + sine, target_assign="rotated", dir_head=True) on the tiny golden batch with
   one car per frame on a slice of the anchor grid in front of the camera: L_dir and acc before / after, AOS against the
   `bbox` AP with and without the head's decode.
Method of tools/bench_assign.py: per arm and round --round-launches calls back to back between two device events, the arms
alternated round by round; reported: median [min, max] over the rounds.  No threshold is set on these numbers.
usage: python tools/bench_dir_head.py [--rounds 20] [--round-launches 50] [--steps 0] [--fit 0] [--out FILE]"""
import argparse
import math
import os
import statistics
import sys
from dataclasses import replace

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
ap.add_argument("--fit", type=int, default=0)
ap.add_argument("--out")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_dir_head.py needs cuda:0 (there is no CPU path to measure)")
if args.rounds < 5 or args.rounds * args.round_launches < 50:
    sys.exit("at least 5 rounds and 50 timed launches per arm")
lib = _lib.load()
st = _lib.raw_stream()
H, W, C = 200, 176, 768
S = H * W
IC_BYTES = 256 << 20
rng = np.random.default_rng(3)
anchors = torch.from_numpy(np.ascontiguousarray(T.generate_anchors("Car").reshape(-1, 7))).to(dev)
w_dir = torch.from_numpy((rng.standard_normal((2, C)) * 0.05).astype(np.float32)).to(dev)
b_dir = torch.zeros(2, dtype=torch.float32, device=dev)
w_heads = torch.from_numpy((rng.standard_normal((16, C)) * 0.05).astype(np.float32)).to(dev)
b_heads = torch.zeros(16, dtype=torch.float32, device=dev)
w_packed = torch.empty((16, C), dtype=torch.bfloat16, device=dev)
_lib.call("vn_pack_weight", w_heads.data_ptr(), 16, C, 1, 0, 0, 1, w_packed.data_ptr(), _lib.VN_BF16, st)
arms = []


def forward_arms(tag, B):
    M_ = B * S
    nbytes = M_ * C * 2
    ring = [torch.randn((M_, C), device=dev).to(torch.bfloat16) for _ in range(IC_BYTES // nbytes + 2)]
    logits = torch.empty((B, 2, S), dtype=torch.float32, device=dev)
    prob = torch.empty((B, 2, S), dtype=torch.float32, device=dev)
    reg = torch.empty((B, 14, S), dtype=torch.float32, device=dev)
    turn = {"dir": 0, "heads": 0}

    def fwd(rows):
        _lib.call("vn_dir_head_fwd", rows.data_ptr(), _lib.VN_BF16, C, w_dir.data_ptr(), b_dir.data_ptr(), B, S, logits.data_ptr(), st)

    def heads(rows):
        _lib.call("vn_heads_fwd", rows.data_ptr(), C, w_packed.data_ptr(), b_heads.data_ptr(), B, S, prob.data_ptr(), reg.data_ptr(), st)

    def cold(fn, key):
        def run():
            turn[key] = (turn[key] + 1) % len(ring)
            fn(ring[turn[key]])
        return run
    note = f"{tag} B={B}, {nbytes / 1e6:.0f} MB"
    arms.append(("vn_dir_head_fwd", note, lambda: fwd(ring[0]), nbytes))
    arms.append(("vn_dir_head_fwd cold", f"{note} x {len(ring)}", cold(fwd, "dir"), nbytes))
    arms.append(("vn_heads_fwd", note, lambda: heads(ring[0]), nbytes))
    arms.append(("vn_heads_fwd cold", f"{note} x {len(ring)}", cold(heads, "heads"), nbytes))
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


ring2 = forward_arms("car", 2)
keep = [ring2]
B = 2
logits2 = torch.randn((B, 2, S), device=dev)
d_cat = torch.zeros((B * S, C), dtype=torch.bfloat16, device=dev)
d_w = torch.empty((2, C), dtype=torch.float32, device=dev)
d_b = torch.empty(2, dtype=torch.float32, device=dev)
nb_bwd = lib.vn_dir_head_bwd_workspace_bytes(B, S)
ws_bwd = torch.empty(nb_bwd, dtype=torch.uint8, device=dev)
nb_loss = lib.vn_rpn_dir_loss_workspace_bytes(B, H, W)
ws_loss = torch.empty(nb_loss, dtype=torch.uint8, device=dev)
out2 = torch.empty(2, dtype=torch.float32, device=dev)
for G in (8, 128):
    pos, neg, tgt = car_targets(G)
    d_logits = torch.empty_like(logits2)
    _lib.call("vn_rpn_dir_loss", logits2.data_ptr(), pos.data_ptr(), tgt.data_ptr(), anchors.data_ptr(), B, H, W, math.pi / 4,
              ws_loss.data_ptr(), nb_loss, out2.data_ptr(), d_logits.data_ptr(), st)
    rows_listed = int(((d_logits[:, 0] != 0) | (d_logits[:, 1] != 0)).sum())
    keep += [pos, neg, tgt, d_logits]

    def bwd(g=d_logits):
        _lib.call("vn_dir_head_bwd", g.data_ptr(), ring2[0].data_ptr(), _lib.VN_BF16, C, w_dir.data_ptr(), B, S, d_cat.data_ptr(),
                  _lib.VN_BF16, C, d_w.data_ptr(), d_b.data_ptr(), ws_bwd.data_ptr(), nb_bwd, st)

    def loss(p=pos, t=tgt, g=d_logits):
        _lib.call("vn_rpn_dir_loss", logits2.data_ptr(), p.data_ptr(), t.data_ptr(), anchors.data_ptr(), B, H, W, math.pi / 4,
                  ws_loss.data_ptr(), nb_loss, out2.data_ptr(), g.data_ptr(), st)
    arms.append(("vn_dir_head_bwd", f"car B=2, {G} boxes: {rows_listed} rows", bwd, None))
    arms.append(("vn_rpn_dir_loss", f"car B=2, {G} boxes", loss, None))
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
say(f"== direction head (full Car grid, {S} sites per frame): {args.rounds} alternated rounds of {args.round_launches} calls per arm; "
    f"us per call, median [min, max] over the rounds; GB/s of row bytes at the median ==")
for a, b, _, nbytes in arms:
    v = us[(a, b)]
    bw = f"{nbytes / statistics.median(v) / 1e3:8.0f} GB/s" if nbytes else ""
    say(f"{a:22s} {b:36s} {statistics.median(v):9.2f} [{min(v):8.2f}, {max(v):8.2f}] {bw}")
del keep, ring2
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
    for name, kw in (("per-layer, no head", {}), ("per-layer, dir_head", {"dir_head": True})):
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
        say(f"{name:22s} {statistics.median(v):9.2f} [{min(v):8.2f}, {max(v):8.2f}]")
    del models
    torch.cuda.empty_cache()

if args.fit > 0:
    from oracle import torch_ref as tr
    from voxelnet_amd.evaluate import KittiDetectionEvaluator
    from voxelnet_amd.optim import ClipAdamW
    from voxelnet_amd.predict import TRAINED_DECODE, BoxDecoder
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import kitti_ref as K
    M.set_precision("bf16")
    g = np.load(os.path.join(ROOT, "tests", "golden", "middle_tiny_car.npz"))
    lens = [int(x) for x in g["feat_lens"]]
    feats = [f.to(dev) for f in torch.split(torch.from_numpy(g["features"]), lens)]
    coords = [c.to(dev) for c in torch.split(torch.from_numpy(g["coords"]), lens)]
    anc = np.ascontiguousarray(T.generate_anchors("Car")[100:108, 60:72])          # 8 x 12 sites in front of the camera
    a = anc.reshape(-1, 7)
    cx, cy = (a[:, 0].min() + a[:, 0].max()) / 2, (a[:, 1].min() + a[:, 1].max()) / 2
    labels = [[K.label_line("Car", [cx - 0.3, cy + 0.2, -1.7, 1.5, 1.6, 3.9, 0.2 - math.pi], digits=6)],
              [K.label_line("Car", [cx + 0.2, cy - 0.1, -1.7, 1.6, 1.7, 4.2, 2.0], digits=6)]]
    batch = (["000000", "000001"], labels, feats, None, coords, None, None)
    torch.manual_seed(7)
    m = M.RPN3D("Car", cls_loss="focal", yaw_loss="sin", target_assign="rotated", dir_head=True)
    m.load_state_dict(tr.make_state_dict("Car"), strict=False)
    m.feature_net._grid = replace(m.feature_net._grid, H=16, W=24)
    m = m.to(dev).train()
    m.__dict__["_targets"] = T.TargetGenerator("Car", dev, anchors=anc, assign="rotated", keep_heading=True)
    dec = BoxDecoder("Car", dev, anchors=anc)
    opt = ClipAdamW(list(m.parameters()), lr=1e-3, max_norm=5.0)

    def score(tag):
        """a forward without gradients, then the same maps decoded with and without the head's logits.  The forward is a
        train-mode one (batch statistics, the regime the fit ran in): a few dozen steps do not settle the running statistics"""
        with torch.no_grad():
            prob, delta = m.detect(feats, coords)
        kw = dict(TRAINED_DECODE, score_thres=0.3)
        res = {}
        for name, extra in (("with the head's decode", dict(dir_logits=m.last_dir_logits, dir_offset=m.dir_offset)), ("without", {})):
            ev = KittiDetectionEvaluator("Car", dev)
            ev.update(*dec.decode_device(prob, delta, top_k=ev.top_k, **kw, **extra), labels)
            r = ev.compute()
            res[name] = (r["bbox"]["all"], r["aos"]["all"], r["n_det"])
        say(f"{tag}: " + "; ".join(f"{k}: bbox AP {v[0]:.4f}, AOS {v[1]:.4f}, {v[2]} detections" for k, v in res.items()))
    first = None
    for i in range(args.fit):
        out = m.train_step(batch, dev, opt)
        if i == 0:
            first = (float(out[2].detach()), float(m.last_dir[0]), float(m.last_dir[1]))
        opt.zero_grad(set_to_none=True)
    with torch.no_grad():
        out = m(batch, dev)
    say(f"== {args.fit} ClipAdamW steps (lr 1e-3, focal + sine, rotated assignment, dir_head) on the tiny golden batch, one car per frame ==")
    say(f"loss {first[0]:.4f} -> {float(out[2]):.4f}; L_dir {first[1]:.4f} -> {float(m.last_dir[0]):.4f}; acc {first[2]:.3f} -> {float(m.last_dir[1]):.3f}")
    score("after the fit")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
