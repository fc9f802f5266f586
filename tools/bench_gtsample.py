"""The ground-truth database sampling stage alone (csrc/gtsample.hip, voxelnet_amd/gtsample.py):
  1. `vn_points_in_boxes` (with counts), `vn_gt_paste` and `vn_gt_paste_visible` on a 20k-point car frame and the
     ~300k-point dense frame with 0 / 15 / 128 boxes in the table and 1,200 object points: time per call in a
     back-to-back train of calls (device events; the table and the object points staged once, so the kernels alone),
     against the HBM floor of 32 B per point;
  2. the input pipeline's stage per batch (DeviceCollate.launch + concat + finish, batch of 2 car frames from memory)
     with gt_sampler off, on and on with a `Visibility` (the occlusion-consistent paste), interleaved: the host's time
     per batch and the pipeline stream's busy time per batch (events on the pipeline stream around the batch's work) —
     what has to stay inside one train step;
  3. the host's share: one draw per sample.
The database is cut on the device from 16 synthetic frames (6 cars each).
usage: python tools/bench_gtsample.py [--out FILE]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import numpy as np
import torch
from voxelnet_amd import _lib
from voxelnet_amd import dataset as D
from voxelnet_amd import gtsample as G
from voxelnet_amd import synth

dev = "cuda:0"
HBM = 6.29e12          # B/s, measured float4 copy on the MI355X
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


def frame(f):
    return synth.synth_cloud("Car", 6000, synth.frame_seed(2, f), 2.3, 35), synth.synth_labels("Car", 6, f)


db = G.GTDatabase.build([(f"{f:06d}", *frame(f)) for f in range(8, 24)], dev, ("Car",))
say(f"database: {len(db)} objects of 16 frames, {sum(e.points.shape[0] >= 5 for e in db.entries)} with >= 5 points")

say("== kernels alone: us per call in a train of 300 calls; 1.5 m x 1.6 m x 4 m boxes over the crop, 1,200 object points ==")
rng = np.random.default_rng(0)
obj = torch.from_numpy(frame(0)[0][:1200].copy()).to(dev)
for name, cloud in (("car 20k", synth.workload_frames(2, batch=1)[0]), ("dense 300k", synth.workload_frames(5, batch=1)[0])):
    pts = torch.from_numpy(cloud).to(dev)
    n, m = pts.shape[0], obj.shape[0]
    out = torch.empty((n + m, 4), dtype=torch.float32, device=dev)
    index = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(128, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().vn_gt_paste_workspace_bytes(n), dtype=torch.uint8, device=dev)
    floor = 32.0 * n / HBM * 1e6
    for g in (0, 15, 128):
        boxes = np.stack([rng.uniform(2, 68, g), rng.uniform(-38, 38, g), rng.uniform(-2.5, -1.5, g), np.full(g, 1.5), np.full(g, 1.6),
                          np.full(g, 4.0), rng.uniform(-1.5, 1.5, g)], 1).reshape(g, 7)
        tab = torch.from_numpy(G.box_table(boxes).view(np.uint8).copy()).to(dev) if g else None
        tp = tab.data_ptr() if g else None
        us_i = train_of_launches(lambda: _lib.call("vn_points_in_boxes", pts.data_ptr(), n, tp, g, index.data_ptr(),
                                                   counts.data_ptr(), _lib.raw_stream()), 300)
        us_p = train_of_launches(lambda: _lib.call("vn_gt_paste", pts.data_ptr(), n, tp, g, obj.data_ptr(), m, out.data_ptr(),
                                                   n + m, count.data_ptr(), ws.data_ptr(), ws.numel(), _lib.raw_stream()), 300)
        say(f"{name:10s} n = {n:6d}  {g:3d} boxes: vn_points_in_boxes {us_i:7.2f} us   vn_gt_paste (3 launches) {us_p:7.2f} us"
            f"   removed {n + m - int(count.item()):6d}   HBM floor (32 B/point at 6.29 TB/s) {floor:5.2f} us")
        # the occlusion-consistent paste on the same cloud and table: the object points split evenly over the boxes
        # (without boxes there are no objects), the default grid
        mv = m if g else 0
        offsets = np.linspace(0, mv, g + 1).astype(np.int32)
        grid = G.Visibility().grid()
        wsv = torch.empty(_lib.load().vn_gt_paste_visible_workspace_bytes(n, mv, grid), dtype=torch.uint8, device=dev)
        ints = torch.empty(2 + 2 * 128, dtype=torch.int32, device=dev)
        us_v = train_of_launches(lambda: _lib.call(
            "vn_gt_paste_visible", pts.data_ptr(), n, tp, g, obj.data_ptr() if mv else None, mv, offsets.ctypes.data, grid, out.data_ptr(),
            n + m, count.data_ptr(), ints[2:].data_ptr(), ints[130:].data_ptr(), ints.data_ptr(), wsv.data_ptr(), wsv.numel(),
            _lib.raw_stream()), 300)
        stats = ints[:2].cpu().numpy()
        rejected = int((ints[2:2 + g].cpu().numpy() < grid.min_visible).sum())
        say(f"{'':10s}              {g:3d} boxes: vn_gt_paste_visible ({7 if mv else 4} launches, 512 x 64 x 4 bins) {us_v:7.2f} us"
            f"   removed by a box {stats[0]:6d}, by shadow only {stats[1]:6d}; {rejected} of {g} objects rejected, "
            f"{n + mv - int(count.item()) - int(stats.sum()):6d} object points dropped")

say("== pipeline stage per batch (2 car frames, 6 cars + DontCare each): gt_sampler off / on (fill to 15 cars) / on with "
    "visibility (the default grid), interleaved ==")
frames = [frame(f) for f in range(2)]
sampler = G.GTSampler(db, per_class={"Car": 15}, min_points=5)
sampler_vis = G.GTSampler(db, per_class={"Car": 15}, min_points=5, visibility=G.Visibility())
ARMS = ("off", "on", "visible")
collates = {"off": D.DeviceCollate(dev, "Car"), "on": D.DeviceCollate(dev, "Car", gt_sampler=sampler),
            "visible": D.DeviceCollate(dev, "Car", gt_sampler=sampler_vis)}
st = collates["off"].stream


def one_batch(c):
    parts = [(f"{i:06d}", None, cloud.copy(), list(lab), None) for i, (cloud, lab) in enumerate(frames)]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(st)
    launched = c.concat(c.launch(parts))
    e.record(st)
    out = c.finish(launched)
    return s, e, out


np.random.seed(0)
host = {a: [] for a in ARMS}
busy = {a: [] for a in ARMS}
labels_out = {a: [] for a in ARMS}
for rnd in range(12):
    for flag in ARMS:
        c = collates[flag]
        for _ in range(3):
            one_batch(c)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(40):
            one_batch(c)
        torch.cuda.synchronize()
        host[flag].append((time.perf_counter() - t0) / 40 * 1e3)
        # stream-busy time of ONE batch with nothing else queued: issue, wait, read the bracket
        one = []
        for _ in range(10):
            torch.cuda.synchronize()
            s, e, out = one_batch(c)
            torch.cuda.synchronize()
            one.append(s.elapsed_time(e))
            labels_out[flag].append(np.mean([len(lab) for lab in out[1]]))
        busy[flag].append(float(np.median(one)))
for flag in ARMS:
    h, b = np.array(host[flag]), np.array(busy[flag])
    say(f"gt_sampler {flag:7s}: {np.mean(labels_out[flag]):5.2f} label lines per sample; wall time per batch, back to back (host enqueue + draw, device keeps up) {h.mean():6.3f} +- {h.std():5.3f} ms;"
        f"  one batch alone, first copy to end of concat on the pipeline stream {b.mean():6.3f} +- {b.std():5.3f} ms   (12 rounds)")
for hi, lo in (("on", "off"), ("visible", "on")):
    dh = np.array(host[hi]) - np.array(host[lo])
    dbusy = np.array(busy[hi]) - np.array(busy[lo])
    say(f"paired difference {hi} - {lo}: wall {dh.mean():+6.3f} +- {dh.std() / np.sqrt(len(dh)):5.3f} ms (s.e.),"
        f"  alone {dbusy.mean():+6.3f} +- {dbusy.std() / np.sqrt(len(dbusy)):5.3f} ms (s.e.)")
np.random.seed(1)
ts, acc = [], []
for i in range(100):
    t0 = time.perf_counter()
    p = sampler.draw(frames[i % 2][1], f"{i % 2:06d}")
    ts.append(time.perf_counter() - t0)
    acc.append(len(p.lines))
say(f"host draw, one sample (9 candidates against 7 + accepted boxes): {np.mean(ts) * 1e3:6.3f} ms, {np.mean(acc):4.1f} objects accepted")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")
