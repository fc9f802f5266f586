"""The part-aware augmentation stage alone (csrc/part_augment.hip, voxelnet_amd/part_augment.py): `vn_part_augment` (three
launches: zero, count, apply) beside `vn_points_in_boxes` (one launch; with the per-box counts it walks the whole table,
without them it stops at the first hit like the count pass here) and `vn_augment_compose` (one launch) on the SAME cloud
and the same number of table entries: n = 20,000 and 120,000 rows, 8 / 32 / 128 entries.

The cloud: car-sized boxes scattered over the crop, a tenth of the rows uniform inside them (spread evenly over the
boxes), the rest uniform over the crop.  The part table has every operation on: each entry drops one pyramid, thins
another (keep 0.5) and swaps a third with its neighbour.  All calls run out of place, so the input is the same for every
launch.  Time per call in a back-to-back train of 200 calls (device events), median [min, max] of 9 rounds in which the
four calls alternate; the tables are staged once (the kernels alone, without the host->device copy of the table).
usage: python tools/bench_part_augment.py [--out FILE]"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "voxelnet-pytorch_amd")]
import numpy as np
import torch
from voxelnet_amd import _lib
from voxelnet_amd import augment as A
from voxelnet_amd import gtsample as G
from voxelnet_amd import part_augment as P

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


def fmt(v):
    return f"{np.median(v):7.2f} [{min(v):7.2f}, {max(v):7.2f}]"


def scene(n, g, rng):
    boxes = np.stack([rng.uniform(2, 68, g), rng.uniform(-38, 38, g), rng.uniform(-2.0, -1.4, g), np.full(g, 1.56), np.full(g, 1.6),
                      np.full(g, 3.9), rng.uniform(-1.5, 1.5, g)], 1)
    per = n // 10 // g
    rows = []
    for b in boxes:
        q = rng.uniform(-0.99, 0.99, (per, 3)) * np.array([b[5] / 2, b[4] / 2, b[3] / 2])
        c, s = np.cos(b[6]), np.sin(b[6])
        rows.append(np.stack([b[0] + q[:, 0] * c - q[:, 1] * s, b[1] + q[:, 0] * s + q[:, 1] * c, b[2] + b[3] / 2 + q[:, 2],
                              rng.uniform(0, 1, per)], 1))
    rows.append(rng.uniform([0, -40, -3, 0], [70.4, 40, 1, 1], (n - per * g, 4)))
    cloud = np.concatenate(rows).astype(np.float32)
    return np.ascontiguousarray(cloud[rng.permutation(n)]), boxes


say("== us per call, median [min, max] of 9 alternated rounds of 200 calls; out of place; tables staged once ==")
rng = np.random.default_rng(0)
for n in (20_000, 120_000):
    for g in (8, 32, 128):
        cloud, boxes = scene(n, g, rng)
        pts = torch.from_numpy(cloud).to(dev)
        dst = torch.empty_like(pts)
        part = P.part_table(boxes)
        for k in range(g):
            part[k]["drop_mask"], part[k]["sparse_mask"], part[k]["swap_mask"] = 1 << (k % 6), 1 << ((k + 1) % 6), 1 << ((k + 2) % 6)
            part[k]["sparse_key"], part[k]["sparse_thresh"], part[k]["sparse_min"] = 1000 + k, 1 << 23, 4
            part[k]["swap_with"] = k ^ 1
        P.check_table(part)
        move = np.zeros(g, dtype=A.MOVE_DTYPE)
        plain = G.box_table(boxes)
        for k in range(g):
            for f in plain.dtype.names:
                move[k][f] = plain[k][f]
            rz = rng.uniform(-0.3, 0.3)
            move[k]["tx"], move[k]["ty"], move[k]["tz"], move[k]["rc"], move[k]["rs"] = *rng.normal(size=3), np.cos(rz), np.sin(rz)
        part_d, move_d, plain_d = (torch.from_numpy(t.view(np.uint8)).to(dev) for t in (part, move, plain))
        aff = _lib.VnAffine(*A.compose_affine(True, 0.4, 1.03, (0.1, 0.2, 0.05)))
        ints = torch.empty(g * 9, dtype=torch.int32, device=dev)
        index = torch.empty(n, dtype=torch.int32, device=dev)
        box_counts = torch.empty(g, dtype=torch.int32, device=dev)
        ws = torch.empty(max(_lib.load().vn_part_augment_workspace_bytes(n, g), 16), dtype=torch.uint8, device=dev)

        def parts():
            _lib.call("vn_part_augment", pts.data_ptr(), n, part_d.data_ptr(), g, None, 0, 0, dst.data_ptr(), ints.data_ptr(),
                      ints.data_ptr() + 4 * g * 6, ws.data_ptr(), ws.numel(), _lib.raw_stream())

        def pib_first():
            _lib.call("vn_points_in_boxes", pts.data_ptr(), n, plain_d.data_ptr(), g, index.data_ptr(), None, _lib.raw_stream())

        def pib_counts():
            _lib.call("vn_points_in_boxes", pts.data_ptr(), n, plain_d.data_ptr(), g, index.data_ptr(), box_counts.data_ptr(),
                      _lib.raw_stream())

        def compose():
            _lib.call("vn_augment_compose", pts.data_ptr(), n, move_d.data_ptr(), g, ctypes.byref(aff), dst.data_ptr(), _lib.raw_stream())

        parts()
        torch.cuda.synchronize()
        stats = ints[g * 6:].view(g, 3).sum(0).tolist()
        owned = int(ints[:g * 6].sum())
        t = {"part": [], "pib": [], "pibc": [], "compose": []}
        for rnd in range(9):
            t["part"].append(train_of_launches(parts, 200))
            t["pib"].append(train_of_launches(pib_first, 200))
            t["pibc"].append(train_of_launches(pib_counts, 200))
            t["compose"].append(train_of_launches(compose, 200))
        say(f"n = {n:6d}  {g:3d} entries ({owned} rows owned; dropped / thinned / swapped {stats}):  vn_part_augment {fmt(t['part'])}"
            f"   vn_points_in_boxes first hit {fmt(t['pib'])}, with counts {fmt(t['pibc'])}   vn_augment_compose {fmt(t['compose'])}"
            f"   ratio to vn_points_in_boxes {np.median(t['part']) / np.median(t['pib']):4.2f} (first hit), "
            f"{np.median(t['part']) / np.median(t['pibc']):4.2f} (with counts)   HBM floor of one 32 B/row pass {32.0 * n / HBM * 1e6:5.2f} us")
if "--out" in sys.argv:
    path = sys.argv[sys.argv.index("--out") + 1]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").write("\n".join(lines) + "\n")
