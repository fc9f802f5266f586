"""The augmentation stage alone (csrc/augment.hip, voxelnet_amd/augment.py):
  1. `vn_augment_points` per mode on a 20k-point car frame and the ~300k-point dense frame, 16 boxes in the table:
     time per launch in a back-to-back train of launches (device events), against the HBM floor of 32 B per point;
  2. the input pipeline's stage per batch (DeviceCollate.launch + concat + finish, batch of 2 car frames from memory)
     with augment=False and augment=True, interleaved: the host's time per batch and the pipeline stream's busy time
     per batch (events on the pipeline stream around the batch's work);
  3. the composed recipe: `vn_augment_compose` (one launch) against the three existing launches run back to back
     (boxes -> rotate -> scale) on both clouds with 7 and 128 table entries, median [min, max] of alternated rounds,
     and the pipeline stage per batch with augment=True against augment=ComposeRecipe().
usage: python tools/bench_augment.py [--out FILE]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import numpy as np
import torch
from voxelnet_amd import augment as A
from voxelnet_amd import dataset as D
from voxelnet_amd import synth

dev = "cuda:0"
HBM = 6.29e12          # B/s, measured float4 copy on the MI355X
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def draw(labels, mode):
    want = {"scale": lambda c: c < 4, "rotate": lambda c: 4 <= c < 7, "boxes": lambda c: c >= 7}[mode]
    for seed in range(1000):
        np.random.seed(seed)
        if want(np.random.randint(0, 10)):
            np.random.seed(seed)
            return A.draw_augmentation(labels)


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


say("== kernel alone: us per launch in a train of 500 launches (out of place: the input stays), 16 cars + DontCare in the table ==")
labels = synth.synth_labels("Car", 16, 3)
for name, cloud in (("car 20k", synth.workload_frames(2, batch=1)[0]), ("dense 300k", synth.workload_frames(5, batch=1)[0])):
    pts = torch.from_numpy(cloud).to(dev)
    n = pts.shape[0]
    dst = torch.empty_like(pts)
    floor = 32.0 * n / HBM * 1e6
    for mode in ("boxes", "rotate", "scale"):
        p = draw(labels, mode)
        if mode == "boxes":      # the table staged once: the kernel alone, without the 1-KB copy in front of it
            tab = torch.from_numpy(p.table.view(np.uint8)).to(dev)
            from voxelnet_amd import _lib
            fn = lambda: _lib.call("vn_augment_points", pts.data_ptr(), n, 0, tab.data_ptr(), len(p.table), 1.0, 0.0, 1.0,  # noqa: E731
                                   dst.data_ptr(), _lib.raw_stream())
        else:
            fn = lambda: A.augment_points_device(pts, p, out=dst)  # noqa: E731
        us = train_of_launches(fn, 500)
        say(f"{name:10s} n = {n:6d}  {mode:6s}: {us:7.2f} us / launch   HBM floor (32 B/point at 6.29 TB/s) {floor:5.2f} us"
            f"   -> {32.0 * n / (us * 1e-6) / 1e12:5.2f} TB/s effective")
    p = draw(labels, "boxes")
    us = train_of_launches(lambda: A.augment_points_device(pts, p, out=dst), 500)
    say(f"{name:10s} n = {n:6d}  boxes through augment_points_device (pinned table + copy + launch): {us:7.2f} us / call")

say("== pipeline stage per batch (2 car frames, 6 cars + DontCare each): augment=False vs True, interleaved ==")
frames = [(synth.synth_cloud("Car", 6000, synth.frame_seed(2, f), 2.3, 35), synth.synth_labels("Car", 6, f)) for f in range(2)]
collates = {False: D.DeviceCollate(dev, "Car"), True: D.DeviceCollate(dev, "Car", augment=True)}
st = collates[False].stream


def one_batch(c):
    parts = [(f"{i:06d}", None, cloud.copy(), list(lab), None) for i, (cloud, lab) in enumerate(frames)]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(st)
    launched = c.concat(c.launch(parts))
    e.record(st)
    out = c.finish(launched)
    return s, e, out


np.random.seed(0)
host = {False: [], True: []}
busy = {False: [], True: []}
for rnd in range(12):
    for flag in (False, True):
        c = collates[flag]
        for _ in range(3):
            one_batch(c)
        torch.cuda.synchronize()
        evs = []
        t0 = time.perf_counter()
        for _ in range(40):
            evs.append(one_batch(c)[:2])
        torch.cuda.synchronize()
        host[flag].append((time.perf_counter() - t0) / 40 * 1e3)
        # stream-busy time of ONE batch with nothing else queued: issue, wait, read the bracket
        one = []
        for _ in range(10):
            torch.cuda.synchronize()
            s, e, _ = one_batch(c)
            torch.cuda.synchronize()
            one.append(s.elapsed_time(e))
        busy[flag].append(float(np.median(one)))
for flag in (False, True):
    h, b = np.array(host[flag]), np.array(busy[flag])
    say(f"augment={str(flag):5s}: wall time per batch, back to back (host enqueue + draw, device keeps up) {h.mean():6.3f} +- {h.std():5.3f} ms;"
        f"  one batch alone, first copy to end of concat on the pipeline stream {b.mean():6.3f} +- {b.std():5.3f} ms   (12 rounds)")
dh = np.array(host[True]) - np.array(host[False])
db = np.array(busy[True]) - np.array(busy[False])
say(f"paired difference True - False: wall {dh.mean():+6.3f} +- {dh.std() / np.sqrt(len(dh)):5.3f} ms (s.e.),"
    f"  alone {db.mean():+6.3f} +- {db.std() / np.sqrt(len(db)):5.3f} ms (s.e.)")
# the host's share: the draw + the moved labels per sample, by mode
for mode in ("boxes", "rotate", "scale"):
    lab = frames[0][1]
    np.random.seed(1)
    ts = []
    while len(ts) < 100:
        t0 = time.perf_counter()
        p = A.draw_augmentation(lab)
        A.augment_labels(lab, p)
        if p.mode == mode:
            ts.append(time.perf_counter() - t0)
    say(f"host draw + labels, one sample, {mode:6s}: {np.mean(ts) * 1e3:6.3f} ms")

# ---------------------------------------------------------------------------------------------------------------------
# the composed recipe (vn_augment_compose): one launch against the three existing ones run back to back
# ---------------------------------------------------------------------------------------------------------------------
import ctypes  # noqa: E402

from voxelnet_amd import _lib  # noqa: E402
from voxelnet_amd import gtsample as G  # noqa: E402


def fmt(v):
    return f"{np.median(v):7.2f} [{min(v):7.2f}, {max(v):7.2f}]"


say("== composed launch vs boxes -> rotate -> scale back to back: us per cloud, median [min, max] of 9 alternated rounds of 200 ==")
rng = np.random.default_rng(0)
for name, cloud in (("car 20k", synth.workload_frames(2, batch=1)[0]), ("dense 300k", synth.workload_frames(5, batch=1)[0])):
    pts = torch.from_numpy(cloud).to(dev)
    n = pts.shape[0]
    dst = torch.empty_like(pts)
    for g in (7, 128):
        boxes = np.stack([rng.uniform(2, 68, g), rng.uniform(-38, 38, g), rng.uniform(-2.0, -1.4, g), np.full(g, 1.56), np.full(g, 1.6),
                          np.full(g, 3.9), rng.uniform(-1.5, 1.5, g)], 1)
        old = np.zeros(g, dtype=A.BOX_DTYPE)
        new = np.zeros(g, dtype=A.MOVE_DTYPE)
        unmoved = G.box_table(boxes)
        for i, b in enumerate(boxes):
            rz, t = rng.uniform(-0.3, 0.3), rng.normal(size=3)
            lo, hi = A.box_bounds(b)
            old[i] = (lo, hi, tuple(t), np.cos(rz), np.sin(rz))
            for f in unmoved.dtype.names:
                new[i][f] = unmoved[i][f]
            new[i]["tx"], new[i]["ty"], new[i]["tz"], new[i]["rc"], new[i]["rs"] = t[0], t[1], t[2], np.cos(rz), np.sin(rz)
        old_d = torch.from_numpy(old.view(np.uint8)).to(dev)
        new_d = torch.from_numpy(new.view(np.uint8)).to(dev)
        aff = _lib.VnAffine(*A.compose_affine(True, 0.4, 1.03, (0.1, 0.2, 0.05)))
        c, s = float(np.cos(0.4)), float(np.sin(0.4))

        def three():
            st = _lib.raw_stream()
            _lib.call("vn_augment_points", pts.data_ptr(), n, 0, old_d.data_ptr(), g, 1.0, 0.0, 1.0, dst.data_ptr(), st)
            _lib.call("vn_augment_points", dst.data_ptr(), n, 1, None, 0, c, s, 1.0, dst.data_ptr(), st)
            _lib.call("vn_augment_points", dst.data_ptr(), n, 2, None, 0, 1.0, 0.0, 1.03, dst.data_ptr(), st)

        def one():
            _lib.call("vn_augment_compose", pts.data_ptr(), n, new_d.data_ptr(), g, ctypes.byref(aff), dst.data_ptr(), _lib.raw_stream())

        t3, t1 = [], []
        for rnd in range(9):
            t3.append(train_of_launches(three, 200))
            t1.append(train_of_launches(one, 200))
        say(f"{name:10s} n = {n:6d}  {g:3d} entries: three launches {fmt(t3)} us   composed {fmt(t1)} us"
            f"   (HBM floor of one pass {32.0 * n / HBM * 1e6:5.2f} us)")

say("== pipeline stage per batch (2 car frames, 6 cars + DontCare each): augment=True vs augment=ComposeRecipe(), interleaved ==")
collates["compose"] = D.DeviceCollate(dev, "Car", augment=A.ComposeRecipe())
host2 = {True: [], "compose": []}
busy2 = {True: [], "compose": []}
np.random.seed(0)
for rnd in range(12):
    for flag in (True, "compose"):
        c = collates[flag]
        for _ in range(3):
            one_batch(c)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(40):
            one_batch(c)
        torch.cuda.synchronize()
        host2[flag].append((time.perf_counter() - t0) / 40 * 1e3)
        alone = []
        for _ in range(10):
            torch.cuda.synchronize()
            s, e, _ = one_batch(c)
            torch.cuda.synchronize()
            alone.append(s.elapsed_time(e))
        busy2[flag].append(float(np.median(alone)))
for flag in (True, "compose"):
    say(f"augment={str(flag):8s}: wall per batch, back to back, ms {fmt(host2[flag])};  one batch alone on the pipeline stream, ms {fmt(busy2[flag])}"
        "   (median [min, max] of 12 rounds)")
lab = frames[0][1]
np.random.seed(1)
ts = []
for _ in range(200):
    t0 = time.perf_counter()
    p = A.draw_compose(lab, A.ComposeRecipe())
    A.compose_labels(lab, p)
    ts.append(time.perf_counter() - t0)
say(f"host draw_compose + compose_labels, one sample (6 cars + DontCare): {np.median(ts) * 1e3:6.3f} ms")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")
