"""The two calls of csrc/tta.hip alone: `vn_pool_merge` and `vn_box_vote` per launch, with `vn_box_nms`
(rotated, 0.1) on the same merged pool timed beside them in the same process.  B = 2, V in {1, 2, 4} views, V * K in
{1024, 4096} merged rows, P = 64 kept rows; clustered scenes — objects on a 6 m pitch, 25 jittered candidates per object
and view, every third turned by pi, seen through each view.  Times are per launch in a back-to-back train of launches
(device events), raw library calls on preallocated buffers.  No threshold is set on these numbers.
usage: python tools/bench_tta.py [--out FILE]"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import numpy as np
import torch
from voxelnet_amd import _lib

dev = "cuda:0"
B, P, NMS_THRES, VOTE_THRES, PER = 2, 64, 0.1, 0.5, 25
VIEWS = [(1.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (1.0, math.pi / 8, float(np.float32(1.05))), (-1.0, -math.pi / 8, float(np.float32(0.95)))]
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def train_of_launches(fn, n):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3          # us


def pools(V, K, seed):
    """(V,B,K,7) boxes in each view's coordinates, (V,B,K) scores descending per view, (V,B) counts"""
    rng = np.random.default_rng(seed)
    n_obj = max(1, K // PER)
    slots = np.array([(2.0 + 6.0 * ix, -39.0 + 6.0 * iy) for iy in range(14) for ix in range(12)])[:n_obj]
    boxes, scores = np.zeros((V, B, K, 7), np.float32), np.zeros((V, B, K), np.float32)
    counts = np.zeros((V, B), np.int32)
    for b in range(B):
        obj = np.concatenate([slots + rng.uniform(-0.5, 0.5, slots.shape), np.full((len(slots), 1), -1.0),
                              np.tile([1.5, 1.6, 3.9], (len(slots), 1)), rng.uniform(-math.pi, math.pi, (len(slots), 1))], axis=1)
        for v, (fy, angle, f) in enumerate(VIEWS[:V]):
            q = np.repeat(obj, PER, axis=0)[:K]
            q[:, :2] += rng.normal(0.0, 0.15, (len(q), 2))
            q[:, 3:6] *= 1.0 + rng.normal(0.0, 0.03, (len(q), 3))
            q[:, 6] += rng.normal(0.0, 0.05, len(q)) + np.where(np.arange(len(q)) % 3 == 2, math.pi, 0.0)
            c, s = math.cos(angle), math.sin(angle)
            x, y = q[:, 0], fy * q[:, 1]
            q[:, 0], q[:, 1], q[:, 6] = x * c + y * s, -(x * s) + y * c, fy * q[:, 6] - angle
            q[:, :6] *= f
            boxes[v, b, :len(q)] = q[rng.permutation(len(q))]
            scores[v, b, :len(q)] = np.sort(rng.uniform(0.3, 1.0, len(q)).astype(np.float32))[::-1]
            counts[v, b] = len(q)
    return [torch.from_numpy(a).to(dev) for a in (boxes, scores, counts)]


lib = _lib.load()
say(f"== csrc/tta.hip: us per launch in a train of 200 launches, B = {B}, P = {P}, NMS at {NMS_THRES}, vote at {VOTE_THRES}; "
    f"build {lib.vn_build_id().decode()} ==")
for rows in (1024, 4096):
    for V in (1, 2, 4):
        K = rows // V
        boxes, scores, counts = pools(V, K, 7)
        views = np.ascontiguousarray(np.array(VIEWS[:V], dtype=np.float64))
        mb = torch.zeros((B, rows, 7), dtype=torch.float32, device=dev)
        ms = torch.zeros((B, rows), dtype=torch.float32, device=dev)
        src = torch.zeros((B, rows), dtype=torch.int32, device=dev)
        mc = torch.zeros(B, dtype=torch.int32, device=dev)
        keep = torch.zeros((B, P), dtype=torch.int32, device=dev)
        kc = torch.zeros(B, dtype=torch.int32, device=dev)
        ob = torch.zeros((B, P, 7), dtype=torch.float32, device=dev)
        os_ = torch.zeros((B, P), dtype=torch.float32, device=dev)
        om = torch.zeros((B, P), dtype=torch.int32, device=dev)
        oc = torch.zeros(B, dtype=torch.int32, device=dev)
        nb = max(lib.vn_pool_merge_workspace_bytes(V, B, K), lib.vn_box_nms_workspace_bytes(B, rows),
                 lib.vn_box_vote_workspace_bytes(B, rows, P, V))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)

        def merge():
            _lib.call("vn_pool_merge", boxes.data_ptr(), scores.data_ptr(), counts.data_ptr(), views.ctypes.data, V, B, K, mb.data_ptr(),
                      ms.data_ptr(), src.data_ptr(), mc.data_ptr(), ws.data_ptr(), nb, _lib.raw_stream())

        def nms():
            _lib.call("vn_box_nms", mb.data_ptr(), mc.data_ptr(), B, rows, _lib.VN_NMS_ROTATED, NMS_THRES, P, keep.data_ptr(), kc.data_ptr(),
                      ws.data_ptr(), nb, _lib.raw_stream())

        def vote(wm, sm):
            _lib.call("vn_box_vote", mb.data_ptr(), ms.data_ptr(), mc.data_ptr(), src.data_ptr(), K, keep.data_ptr(), kc.data_ptr(), B, rows,
                      P, V, VOTE_THRES, wm, sm, ob.data_ptr(), os_.data_ptr(), om.data_ptr(), oc.data_ptr(), ws.data_ptr(), nb,
                      _lib.raw_stream())

        us_merge = train_of_launches(merge, 200)
        us_nms = train_of_launches(nms, 200)
        us_vote = train_of_launches(lambda: vote(_lib.VN_VOTE_W_SCORE_IOU, _lib.VN_VOTE_S_VIEW_MEAN), 200)
        us_vote_s = train_of_launches(lambda: vote(_lib.VN_VOTE_W_SCORE, _lib.VN_VOTE_S_KEEP), 200)
        torch.cuda.synchronize()
        say(f"V {V}  V*K {rows:4d}:  vn_pool_merge {us_merge:8.1f} us   vn_box_nms {us_nms:8.1f} us   vn_box_vote {us_vote:8.1f} us "
            f"(score, keep: {us_vote_s:8.1f} us)   pool {mc.tolist()}  kept {kc.tolist()}  mean members {float(om.sum()) / max(1, int(oc.sum())):.1f}")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")
