"""The point shuffle of the input pipeline (csrc/shuffle.hip, voxelnet_amd/shuffle.py):
  1. `vn_permute_points` and `vn_shuffle_points` on the 20k-point car frame and the ~300k-point dense frame: time per
     call in a back-to-back train of calls (device events; the index table staged once, so the kernels alone), against
     the HBM floor of 32 B per point;
  2. the input pipeline's stage per batch (DeviceCollate.launch + concat + finish, batch of 2 car frames held in memory)
     for shuffle_points = True (arm 0: the host shuffle), "index" (arm 1) and "device" (arm 2), interleaved, >= 12 rounds:
     the wall time per batch back to back, the HOST time spent inside `launch` alone, and the pipeline stream's busy time
     of one batch with nothing else queued;
  3. the host's share per sample: np.random.shuffle of the cloud, the index draw, the key draw, the pinned staging.
With --ab DIR/TAG every round of every arm is also written as DIR/TAG_{wall,host,busy}_<arm>_<round>.json
({"value": milliseconds}) — the files `tools/ab_stats.py TAG_wall DIR` reads (its verdict column is worded for a
throughput: for these millisecond values a NEGATIVE paired difference is the faster arm).
usage: python tools/bench_shuffle.py [--rounds N] [--out FILE] [--ab DIR/TAG]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import numpy as np
import torch
from voxelnet_amd import _lib
from voxelnet_amd import dataset as D
from voxelnet_amd import shuffle as S
from voxelnet_amd import synth

dev = "cuda:0"
HBM = 6.29e12          # B/s, measured float4 copy on the MI355X
ROUNDS = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 12
AB = sys.argv[sys.argv.index("--ab") + 1] if "--ab" in sys.argv else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def train_of_launches(fn, n):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3          # us


say("== kernels alone: us per call in a train of 300 calls ==")
keys = np.array([1, 2, 3, 4, 5, 6], dtype=np.uint32)
for name, cloud in (("car 20k", synth.workload_frames(2, batch=1)[0]), ("dense 300k", synth.workload_frames(5, batch=1)[0])):
    pts = torch.from_numpy(cloud).to(dev)
    n = pts.shape[0]
    out = torch.empty_like(pts)
    index = torch.from_numpy(np.random.default_rng(0).permutation(n).astype(np.int32)).to(dev)
    us_p = train_of_launches(lambda: _lib.call("vn_permute_points", pts.data_ptr(), n, index.data_ptr(), out.data_ptr(), _lib.raw_stream()), 300)
    us_s = train_of_launches(lambda: _lib.call("vn_shuffle_points", pts.data_ptr(), n, keys.ctypes.data, out.data_ptr(), _lib.raw_stream()), 300)
    say(f"{name:10s} n = {n:6d}: vn_permute_points {us_p:7.2f} us   vn_shuffle_points {us_s:7.2f} us"
        f"   HBM floor (32 B/point at 6.29 TB/s) {32.0 * n / HBM * 1e6:5.2f} us")

say(f"== pipeline stage per batch (2 car frames held in memory): shuffle_points True / 'index' / 'device', interleaved, {ROUNDS} rounds ==")
frames = [(c, synth.synth_labels("Car", 6, f)) for f, c in enumerate(synth.workload_frames(2, batch=2))]
ARMS = [True, "index", "device"]
collates = [D.DeviceCollate(dev, "Car", shuffle_points=a) for a in ARMS]
st = collates[0].stream
in_launch = [0.0]


def one_batch(c):
    parts = [(f"{i:06d}", None, cloud.copy(), list(lab), None) for i, (cloud, lab) in enumerate(frames)]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(st)
    t0 = time.perf_counter()
    launched = c.launch(parts)
    in_launch[0] += time.perf_counter() - t0
    launched = c.concat(launched)
    e.record(st)
    out = c.finish(launched)
    return s, e, out


np.random.seed(0)
wall = [[] for _ in ARMS]
host = [[] for _ in ARMS]
busy = [[] for _ in ARMS]
for rnd in range(ROUNDS):
    for k, c in enumerate(collates):
        for _ in range(3):
            one_batch(c)
        torch.cuda.synchronize()
        in_launch[0] = 0.0
        t0 = time.perf_counter()
        for _ in range(40):
            one_batch(c)
        torch.cuda.synchronize()
        wall[k].append((time.perf_counter() - t0) / 40 * 1e3)
        host[k].append(in_launch[0] / 40 * 1e3)
        # stream-busy time of ONE batch with nothing else queued: issue, wait, read the bracket
        one = []
        for _ in range(10):
            torch.cuda.synchronize()
            s, e, _ = one_batch(c)
            torch.cuda.synchronize()
            one.append(s.elapsed_time(e))
        busy[k].append(float(np.median(one)))
        if AB:
            os.makedirs(os.path.dirname(os.path.abspath(AB)), exist_ok=True)
            for what, v in (("wall", wall), ("host", host), ("busy", busy)):
                with open(f"{AB}_{what}_{k}_{rnd}.json", "w") as f:
                    f.write(json.dumps({"value": v[k][-1], "arm": repr(ARMS[k])}) + "\n")
if AB:
    for what in ("wall", "host", "busy"):
        open(f"{AB}_{what}_arms.txt", "w").write("\n".join(f"shuffle_points={a!r}" for a in ARMS) + "\n")
for k, a in enumerate(ARMS):
    w, h, b = np.array(wall[k]), np.array(host[k]), np.array(busy[k])
    say(f"shuffle_points={a!r:9}: wall per batch, back to back {w.mean():6.3f} +- {w.std(ddof=1):5.3f} ms;  host time inside launch "
        f"{h.mean():6.3f} +- {h.std(ddof=1):5.3f} ms;  one batch alone on the pipeline stream {b.mean():6.3f} +- {b.std(ddof=1):5.3f} ms")
for k in (1, 2):
    d = [np.array(v[k]) - np.array(v[0]) for v in (wall, host, busy)]
    say(f"paired difference {ARMS[k]!r} - True ({ROUNDS} rounds, mean +- s.e.): " + ",  ".join(
        f"{what} {x.mean():+6.3f} +- {x.std(ddof=1) / np.sqrt(len(x)):5.3f} ms" for what, x in zip(("wall", "host in launch", "alone"), d)))

say("== the host's share per sample (car frame), ms ==")
cloud = frames[0][0]
n = cloud.shape[0]
np.random.seed(1)


def host_ms(fn, reps=30):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


work = cloud.copy()
say(f"n = {n}: np.random.shuffle(cloud) {host_ms(lambda: np.random.shuffle(work)):6.3f}   draw_index {host_ms(lambda: S.draw_index(n)):6.3f}"
    f"   draw_keys {host_ms(S.draw_keys):6.3f}   cloud.copy() (the benchmark's own) {host_ms(cloud.copy):6.3f}"
    f"   pin_memory of the cloud {host_ms(lambda: torch.from_numpy(cloud).pin_memory()):6.3f}"
    f"   pin_memory of the index {host_ms(lambda: torch.from_numpy(np.arange(n, dtype=np.int32)).pin_memory()):6.3f}")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")
