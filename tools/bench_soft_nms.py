"""`vn_box_soft_nms` (csrc/soft_nms.hip) per launch — its three methods on the BEV IoU and the Gaussian on the
3D IoU — beside `vn_box_nms` (rotated, 0.1) of the same build on the same pool, in the same process.  B = 2, P = 64 kept rows,
K in {1024, 4096}; clustered scenes — objects on a 6 m pitch, 25 jittered candidates per object, every third turned by pi,
scores in [0.3, 1) descending along the rows.  Times are per launch in a back-to-back train of launches (device events), raw
library calls on preallocated buffers; the calls take turns over ROUNDS rounds, and the median and the smallest round are
reported.  No threshold is set on these numbers.
usage: python tools/bench_soft_nms.py [--out FILE]      (VN_LIB_PATH=... times another build of the library)"""
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import numpy as np
import torch
from voxelnet_amd import _lib

dev = "cuda:0"
B, P, PER, ROUNDS, TRAIN = 2, 64, 25, 5, 100
NMS_THRES, HARD_THRES, SOFT_THRES, SIGMA, FLOOR = 0.1, 0.1, 0.3, 0.5, 0.05
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def train_of_launches(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3          # us


def pool(K, seed):
    """(B,K,7) boxes, (B,K) scores descending along the rows, (B,) counts"""
    rng = np.random.default_rng(seed)
    n_obj = max(1, K // PER)
    slots = np.array([(2.0 + 6.0 * ix, -39.0 + 6.0 * iy) for iy in range(14) for ix in range(12)])[:n_obj]
    boxes, scores = np.zeros((B, K, 7), np.float32), np.zeros((B, K), np.float32)
    counts = np.zeros(B, np.int32)
    for b in range(B):
        obj = np.concatenate([slots + rng.uniform(-0.5, 0.5, slots.shape), np.full((len(slots), 1), -1.0),
                              np.tile([1.5, 1.6, 3.9], (len(slots), 1)), rng.uniform(-math.pi, math.pi, (len(slots), 1))], axis=1)
        q = np.repeat(obj, PER, axis=0)[:K]
        q[:, :2] += rng.normal(0.0, 0.15, (len(q), 2))
        q[:, 3:6] *= 1.0 + rng.normal(0.0, 0.03, (len(q), 3))
        q[:, 6] += rng.normal(0.0, 0.05, len(q)) + np.where(np.arange(len(q)) % 3 == 2, math.pi, 0.0)
        boxes[b, :len(q)] = q[rng.permutation(len(q))]
        scores[b, :len(q)] = np.sort(rng.uniform(0.3, 1.0, len(q)).astype(np.float32))[::-1]
        counts[b] = len(q)
    return [torch.from_numpy(a).to(dev) for a in (boxes, scores, counts)]


lib = _lib.load()
say(f"== csrc/soft_nms.hip: us per launch in a train of {TRAIN} launches, median (smallest) of {ROUNDS} rounds, B = {B}, P = {P}; "
    f"hard at {HARD_THRES}, linear at {SOFT_THRES}, sigma {SIGMA}, min_score {FLOOR}; vn_box_nms rotated at {NMS_THRES}; "
    f"build {lib.vn_build_id().decode()} ==")
for K in (1024, 4096):
    boxes, scores, counts = pool(K, 7)
    keep = torch.zeros((B, P), dtype=torch.int32, device=dev)
    ks = torch.zeros((B, P), dtype=torch.float32, device=dev)
    kc = torch.zeros(B, dtype=torch.int32, device=dev)
    nb = max(lib.vn_box_nms_workspace_bytes(B, K), lib.vn_box_soft_nms_workspace_bytes(B, K))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)

    def nms():
        _lib.call("vn_box_nms", boxes.data_ptr(), counts.data_ptr(), B, K, _lib.VN_NMS_ROTATED, NMS_THRES, P, keep.data_ptr(), kc.data_ptr(),
                  ws.data_ptr(), nb, _lib.raw_stream())

    def soft(method, metric, thres):
        _lib.call("vn_box_soft_nms", boxes.data_ptr(), scores.data_ptr(), counts.data_ptr(), B, K, method, metric, thres, SIGMA, FLOOR, P,
                  keep.data_ptr(), ks.data_ptr(), kc.data_ptr(), ws.data_ptr(), nb, _lib.raw_stream())

    calls = [("vn_box_nms", nms),
             ("soft hard/bev", lambda: soft(_lib.VN_SOFT_HARD, _lib.VN_SOFT_BEV, HARD_THRES)),
             ("soft linear/bev", lambda: soft(_lib.VN_SOFT_LINEAR, _lib.VN_SOFT_BEV, SOFT_THRES)),
             ("soft gaussian/bev", lambda: soft(_lib.VN_SOFT_GAUSSIAN, _lib.VN_SOFT_BEV, SOFT_THRES)),
             ("soft gaussian/3d", lambda: soft(_lib.VN_SOFT_GAUSSIAN, _lib.VN_SOFT_3D, SOFT_THRES))]
    kept = {}
    for name, fn in calls:          # warm up every call, and note what it keeps
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        kept[name] = kc.tolist()
    us = {name: [] for name, _ in calls}
    for _ in range(ROUNDS):
        for name, fn in calls:
            us[name].append(train_of_launches(fn, TRAIN))
    say(f"K {K:4d}  pool {counts.tolist()}")
    for name, _ in calls:
        say(f"    {name:18s} {statistics.median(us[name]):8.1f} us  ({min(us[name]):8.1f})   kept {kept[name]}")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")
