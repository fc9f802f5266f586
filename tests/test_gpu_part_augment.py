"""GPU: the part-aware object augmentation — `vn_part_augment` (csrc/part_augment.hip through voxelnet_amd.part_augment)
against tests/part_augment_ref.py, BIT-EQUAL: NaN points in the same places, every other row by its uint32 view, the
counts and the stats exactly; and `DeviceCollate` / `DeviceBatcher(part_augment=PartRecipe(...))` against a host replay of
the same shuffles and draws (voxel buffers = oracle voxelizer of the restatement's cloud, bit for bit).

What the inputs hold is judged on the CPU, on the restatement alone, by tests/test_part_augment_host.py: the edge points'
owners and pyramids are written down there, and the dense cases are shown to fill every pyramid and to take every branch."""
import numpy as np
import pytest
import torch

import compose_ref as CR
import gtsample_ref as GR
import part_augment_ref as R
import test_gpu_gt_visibility as TV          # its frames, its database (computed once for both files) and its KITTI writer
import visibility_ref as V
from oracle import voxelize as ov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device(cloud, table, inplace=False, gate=None, gate_first=0, gate_min=0):
    """-> (out, counts, stats) of the device, read back; the input tensor and the params are left alone"""
    from voxelnet_amd import part_augment as P
    cloud = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4)
    pts = torch.from_numpy(cloud.copy()).to(DEV)
    params = R.to_params(table)
    before = params.table.copy()
    g = None if gate is None else torch.tensor(list(gate), dtype=torch.int32, device=DEV)
    out, res = P.part_points_device(pts, params, out=pts if inplace else None, gate=g, gate_first=gate_first, gate_min=gate_min)
    assert (out is pts) == inplace
    if not inplace:
        assert pts.cpu().numpy().tobytes() == cloud.tobytes()
    assert params.table.tobytes() == before.tobytes()
    counts, stats = res.counts, res.stats
    assert counts.shape == (len(table), 6) and stats.shape == (len(table), 3) and counts.dtype == stats.dtype == np.int32
    return out.cpu().numpy(), counts, stats


def _check(cloud, table, **gate):
    """the device, out of place and in place, against the restatement -> the restatement's (out, counts, stats)"""
    cloud = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 4)
    want, counts, stats = R.apply(cloud, table, **gate)
    own, _ = R.owner_face(cloud, table, **gate)
    for inplace in (False, True):
        got, c, s = _device(cloud, table, inplace, **gate)
        assert np.array_equal(c, counts), (inplace, c.tolist(), counts.tolist())
        assert np.array_equal(s, stats), (inplace, s.tolist(), stats.tolist())
        assert R.same(got, want), (inplace, int((got.view(np.uint32) != want.view(np.uint32)).any(1).sum()))
        assert got[own < 0].tobytes() == cloud[own < 0].tobytes()          # a row without an owner: a bit copy, payloads included
    return want, counts, stats


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def test_hand_picked_edge_points():
    """the edge points of the host test: untouched, with every pyramid of one box dropped, and with the two boxes swapping
    each pyramid in turn while box A thins and box B drops another one"""
    cloud, boxes, want_owner, want_face = R.edge_points()
    plain = [R.entry(b) for b in boxes]
    out, counts, stats = _check(cloud, plain)
    assert out.tobytes() == cloud.tobytes() and not stats.any()
    assert counts.tolist() == [np.bincount(want_face[want_owner == o], minlength=6).tolist() for o in (0, 1)]
    _, _, stats = _check(cloud, [R.entry(boxes[0], drop=0x3F), R.entry(boxes[1])])
    assert stats.tolist() == [[int((want_owner == 0).sum()), 0, 0], [0, 0, 0]]
    moved = 0
    for f in range(6):
        t = [R.entry(boxes[0], sparse=1 << ((f + 1) % 6), key=77 + f, thresh=1 << 23), R.entry(boxes[1], drop=1 << ((f + 2) % 6))]
        R.pair(t, 0, 1, boxes, f)
        _, counts, stats = _check(cloud, t)
        assert stats[0][2] == counts[0][f] and stats[1][2] == counts[1][f] and stats[1][0] == counts[1][(f + 2) % 6]
        moved += int(stats[:, 2].sum())
    assert moved == int((want_owner >= 0).sum())
    _check(cloud[:0], plain)                                                 # n == 0: zeroed counts and stats
    _check(cloud, [])                                                        # no entries: a copy


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_dense_random_boxes(seed):
    cloud, boxes = R.dense_case(seed)
    assert cloud.shape == (5921, 4)
    table = R.dense_table(boxes)
    want, counts, stats = _check(cloud, table)
    print(f"seed {seed}: counts min {counts.min()}, stats {stats.tolist()}")
    assert counts.min() >= 21 and stats[:, 0].sum() > 0 and stats[:, 1].sum() > 0 and stats[:, 2].sum() > 0
    a, b = _device(cloud, table), _device(cloud, table)                      # two runs give the same bits
    assert R.same(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    # out of place into a caller's buffer
    from voxelnet_amd import part_augment as P
    pts = torch.from_numpy(cloud.copy()).to(DEV)
    buf = torch.full((len(cloud), 4), 7.0, device=DEV)
    out, _ = P.part_points_device(pts, R.to_params(table), out=buf)
    assert out is buf and R.same(buf.cpu().numpy(), want)


def _crowd():
    """128 entries, overlapping in pairs: entry 2k + 1 is entry 2k moved by a metre and turned.  20 points per box, 500
    rows of background; every kind of operation spread over the table"""
    rng = np.random.default_rng(11)
    boxes, rows = [], []
    for k in range(64):
        a = np.array([5.0 + 9.0 * (k % 8), -32.0 + 9.0 * (k // 8), -1.5, 1.6, 1.8, 4.0, rng.uniform(-np.pi, np.pi)])
        b = a + np.array([1.0, 0.5, 0.1, 0.0, 0.2, 0.3, 0.4])
        boxes += [a, b]
    for bx in boxes:
        q = rng.uniform(-0.99, 0.99, (20, 3)) * np.array([bx[5] / 2, bx[4] / 2, bx[3] / 2])
        c, s = np.cos(bx[6]), np.sin(bx[6])
        rows.append(np.stack([bx[0] + q[:, 0] * c - q[:, 1] * s, bx[1] + q[:, 0] * s + q[:, 1] * c, bx[2] + bx[3] / 2 + q[:, 2],
                              rng.uniform(0, 1, 20)], 1))
    rows.append(rng.uniform([0, -40, -3, 0], [80, 40, 1, 1], (500, 4)))
    cloud = np.concatenate(rows).astype(np.float32)
    cloud = np.ascontiguousarray(cloud[rng.permutation(len(cloud))])
    table = [R.entry(bx) for bx in boxes]
    for k, e in enumerate(table):
        if k % 3 == 0:
            e.update(drop_mask=1 << int(rng.integers(6)))
        if k % 3 == 1:
            e.update(sparse_mask=1 << int(rng.integers(6)), sparse_key=int(rng.integers(2 ** 32)), sparse_thresh=1 << 23, sparse_min=3)
    for j in range(0, 128, 4):
        R.pair(table, j, j + 2, boxes, int(rng.integers(6)))
        R.pair(table, j + 1, j + 3, boxes, int(rng.integers(6)))
    return cloud, boxes, table


def test_128_entries_overlapping_in_pairs():
    cloud, boxes, table = _crowd()
    assert len(table) == 128 and len(cloud) == 3060
    both =np.zeros(len(cloud), dtype=bool)
    own, _ = R.owner_face(cloud, table)
    for k in range(64):
        m = R.inside(cloud, table[2 * k]) & R.inside(cloud, table[2 * k + 1])
        assert (own[m] == 2 * k).all()                                       # the lowest index owns the shared points
        both |= m
    assert both.sum() >= 500
    want, counts, stats = _check(cloud, table)
    assert (counts.sum(1) > 0).all() and stats[:, 0].sum() > 50 and stats[:, 1].sum() > 20 and stats[:, 2].sum() > 100
    first_owned = int(np.flatnonzero(own >= 0)[0])
    for rows in (cloud[first_owned:first_owned + 1], cloud[:257], cloud[:256], cloud[:255]):          # n = 1, 257 and the block's edges
        _, c, _ = _check(rows, table)
        assert c.sum() >= 1


def test_gate():
    """entry 1 dead: its points fall to entry 2, a larger box around it; entry 4 dead: the swap of entry 0 with it is void and
    its points have no owner; a gate value equal to gate_min is live; gate = None is every entry live"""
    cloud, boxes = R.dense_case(3)
    around = boxes[1] + np.array([0, 0, -0.2, 0.4, 0.5, 0.5, 0])
    bx = [boxes[0], boxes[1], around] + list(boxes[2:])
    table = [R.entry(b) for b in bx]
    R.pair(table, 0, 4, bx, 1)
    table[2].update(drop_mask=1 << 0)
    table[5].update(sparse_mask=0x3F, sparse_key=5, sparse_thresh=1 << 23, sparse_min=0)
    gate_first, gate_min = 1, 5
    gate = [2, 9, 5, 0, 5, 6, 7, 8]          # entries 1..8: 1 and 4 dead
    assert len(table) == 9 and len(gate) == len(table) - gate_first
    all_live, c_live, s_live = _check(cloud, table)
    want, counts, stats = _check(cloud, table, gate=gate, gate_first=gate_first, gate_min=gate_min)
    assert c_live[1].sum() == 240 and c_live[2].sum() == 0 and counts[1].sum() == 0 and counts[2].sum() == 240
    assert s_live[0][2] == c_live[0][1] > 0 and stats[0][2] == 0 and counts[0][1] == c_live[0][1]          # the void swap
    assert counts[4].sum() == 0 and c_live[4].sum() == 240 and not stats[4].any() and not stats[1].any()
    assert stats[2][0] == counts[2][0] > 0 and stats[5][1] > 0
    # gate = None against a gate that lets everybody live, and against gate_first = G (nobody gated)
    for kw in (dict(gate=[5] * 8, gate_first=1, gate_min=5), dict(gate=[], gate_first=9, gate_min=1 << 30), dict(gate=[0] * 9, gate_first=0, gate_min=0)):
        got, c, s = _device(cloud, table, **kw)
        assert R.same(got, all_live) and np.array_equal(c, c_live) and np.array_equal(s, s_live)


def test_on_a_side_stream_and_wrong_inputs():
    from voxelnet_amd import _lib
    from voxelnet_amd import part_augment as P
    cloud, boxes = R.dense_case(0)
    table = R.dense_table(boxes)
    want, counts, stats = R.apply(cloud, table)
    st = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(st):
        pts = torch.from_numpy(cloud.copy()).pin_memory().to(DEV, non_blocking=True)
        out, keep, res = P.enqueue_part_points(pts, R.to_params(table), out=pts)
    st.synchronize()
    assert out is pts and R.same(out.cpu().numpy(), want) and np.array_equal(res.counts, counts) and np.array_equal(res.stats, stats)
    assert any(t is pts for t in keep)
    p = R.to_params(table)
    for bad in (pts[:, :3], pts.double(), pts[::2]):
        with pytest.raises(_lib.VoxelnetHipError):
            P.part_points_device(bad, p)
    with pytest.raises(_lib.VoxelnetHipError):
        P.part_points_device(pts, p, out=torch.empty((5, 4), device=DEV))
    with pytest.raises(_lib.VoxelnetHipError):
        P.part_points_device(pts, p, gate=torch.zeros(8, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        P.part_points_device(pts, p, gate=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        P.part_points_device(pts, p, gate_first=9)


RECIPE = dict(drop_prob=0.5, sparse_prob=0.5, sparse_keep=0.5, sparse_min=2, swap_prob=0.8)


@pytest.mark.parametrize("f", range(4))
def test_real_frames_with_drawn_recipes(f):
    """the 6,000-point synthetic Car frames, the table drawn by draw_parts (three seeds each)"""
    from voxelnet_amd import part_augment as P
    cloud, labels = TV._frame(f)
    total = np.zeros(3, dtype=np.int64)
    for seed in (3 * f, 3 * f + 1, 3 * f + 2):
        np.random.seed(seed)
        p = P.draw_parts(list(labels), P.PartRecipe(**RECIPE))
        assert len(p.table) == 6
        _, counts, stats = _check(cloud, R.from_params(p))
        total += stats.sum(0)
        print(f"frame {f} seed {seed}: points per entry {counts.sum(1).tolist()}, stats {stats.sum(0).tolist()}")
    assert total.sum() > 0


# ---------------------------------------------------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------------------------------------------------
SEED = 77


def _batches(root, **kw):
    from voxelnet_amd import dataset as D
    np.random.seed(SEED)
    out = list(D.DeviceBatcher(TV._loader(root), DEV, "Car", **kw))
    return out, np.random.random()


@pytest.mark.parametrize("variant", ["alone", "paste", "visibility", "paste+compose"])
def test_part_batcher_matches_the_host_replay(tmp_path, variant):
    """copy -> [paste | visible paste] -> parts -> [compose] -> voxelize against shuffle -> the restatement's draw and paste
    -> draw_parts at its place in the random stream -> the part restatement (on the capacity-sized buffer: the row index keys
    the thinning) -> [the composed restatement] -> oracle voxelizer of the rows that are not NaN points"""
    from voxelnet_amd import augment as A
    from voxelnet_amd import gtsample as G
    from voxelnet_amd import part_augment as P
    root = str(tmp_path / "train")
    TV._make_kitti(root, [0, 1, 2])
    ref_db = list(TV._ref_db())
    recipe = P.PartRecipe(**RECIPE)
    kw = {}
    if variant != "alone":
        vis = G.Visibility() if variant == "visibility" else None
        kw["gt_sampler"] = G.GTSampler(TV._package_db(), per_class=TV.PER_CLASS, visibility=vis)
    if variant == "paste+compose":
        kw["augment"] = A.ComposeRecipe()
    batches, tail = _batches(root, part_augment=recipe, **kw)
    assert [len(b[0]) for b in batches] == [2, 1]
    # the same run without the stage, sample by sample FROM THE SAME np.random STATE (the parts' draw shifts the stream, so
    # a whole second run would hand the later samples another sampler draw); with the composed recipe the draw that
    # moves the labels comes after the parts', so there the replay alone speaks for the labels
    from voxelnet_amd import dataset as D
    plain = None if variant == "paste+compose" else D.DeviceCollate(DEV, "Car", **kw)
    np.random.seed(SEED)
    k = rejected = 0
    total = np.zeros(3, dtype=np.int64)
    for tags, label, feats, nums, coords, rgb, raw in batches:
        for i in range(len(tags)):
            tag = f"{k:06d}"
            assert tags[i] == tag
            cloud, lines = TV._read(root, tag)
            without = None
            if plain is not None:
                state = np.random.get_state()
                without = plain([(tag, None, cloud.copy(), list(lines), None)])
                np.random.set_state(state)
            np.random.shuffle(cloud)
            assert np.array_equal(raw[i], cloud)
            enlarged, buf, gate, acc = lines, cloud, {}, None
            if variant != "alone":
                d = GR.draw(ref_db, lines, tag, TV.PER_CLASS)
                assert len(d["lines"]) >= 5
                enlarged = lines + d["lines"]
            pp = P.draw_parts(enlarged, recipe)                              # after the sampler's draw, before the augmentation's
            assert len(pp.table) == len(enlarged) - 1                        # every line but the frame's DontCare
            if variant == "visibility":
                off = V.offsets_of([e["points"] for line in d["lines"] for e in ref_db if e["line"] == line])
                want = V.paste_visible(cloud, d["boxes"], d["points"], off, V.Grid())
                buf, acc = want["out"], want["accepted"]
                gate = dict(gate=want["visible"].tolist(), gate_first=len(pp.table) - len(d["lines"]), gate_min=V.Grid().min_visible)
                rejected += int((~acc).sum())
            elif variant != "alone":
                buf, _ = GR.paste(cloud, d["boxes"], d["points"])
            moved, counts, stats = R.apply(buf, R.from_params(pp), **gate)
            total += stats.sum(0)
            print(f"sample {k}: {len(pp.table)} entries, points {counts.sum(1).tolist()}, stats {stats.sum(0).tolist()}")
            expect = enlarged
            if variant == "paste+compose":
                dc = CR.draw(enlarged, CR.recipe())
                pr = CR.to_params(dc["table"], dc["affine"])
                pr.boxes_after, pr.has_box = dc["after"], dc["has_box"]
                expect = A.compose_labels(enlarged, pr)
                moved = CR.apply(moved, dc["table"], dc["affine"])
            if acc is not None:
                expect = expect[:len(lines)] + [expect[len(lines) + o] for o in range(len(acc)) if acc[o]]
            assert list(label[i]) == expect
            if without is not None:
                assert list(label[i]) == list(without[1][0])                 # the label lines of the same run without the stage
            ref = ov.voxelize(moved[~np.isnan(moved[:, :3]).any(1)], "Car")
            assert np.array_equal(feats[i].cpu().numpy(), ref["feature_buffer"]), k
            assert np.array_equal(nums[i].cpu().numpy(), ref["number_buffer"]), k
            c = coords[i].cpu().numpy()
            assert np.array_equal(c[:, 1:], ref["coordinate_buffer"]) and (c[:, 0] == i).all()
            if without is not None and stats.any():
                assert not torch.equal(nums[i], without[3][0]) or not torch.equal(feats[i], without[2][0])
            k += 1
    assert k == 3 and np.random.random() == tail                             # the np.random state after the batches
    assert total.sum() > 0 and (variant == "alone" or (total > 0).all()), total          # on the restatement alone: not vacuous
    assert variant != "visibility" or rejected >= 1


def test_part_augment_none_is_the_pipeline_as_it_was(tmp_path, monkeypatch):
    """DeviceBatcher(...) and DeviceBatcher(..., part_augment=None): the same launches, buffers, labels and np.random state;
    with a recipe vn_part_augment runs once per sample"""
    from voxelnet_amd import _lib
    from voxelnet_amd import gtsample as G
    from voxelnet_amd import part_augment as P
    root = str(tmp_path / "kitti")
    TV._make_kitti(root, [0, 1, 2])
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    sampler = G.GTSampler(TV._package_db(), per_class=TV.PER_CLASS)
    runs = []
    for kw in ({}, {"part_augment": None}):
        del calls[:]
        batches, tail = _batches(root, gt_sampler=sampler, **kw)
        runs.append((batches, tail, list(calls)))
    (a, ta, ca), (b, tb, cb) = runs
    assert ta == tb and ca == cb and "vn_part_augment" not in ca
    TV._same_batches(a, b)
    del calls[:]
    _batches(root, gt_sampler=sampler, part_augment=P.PartRecipe())
    assert calls.count("vn_part_augment") == 3
    assert [c for c in calls if c != "vn_part_augment"] == ca                # everything else is launched as before
