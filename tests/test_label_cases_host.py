"""CPU: every case of tests/label_cases.py contains what it was built for — asserted ON THE ORACLE ALONE (oracle/targets.py,
oracle/predict.py, tests/detect_ref.py, tests/eval_ref.py), so that the GPU tests that import the same builders compare the
device on inputs that do exercise partial workgroups, the other classes' constants, the quirky IoU's negative and huge
values, arg-max ties across workgroups and a suppressing NMS.  A case that stops holding a condition fails here; the
remedy is another seed, never a weaker condition.

The oracle for Pedestrian and Cyclist is the Car-pinned code with the other classes' constants (no golden of their own)."""
import numpy as np
import pytest

import detect_ref as D
import eval_ref as R
import label_cases as L
from oracle import predict as op
from oracle import targets as ot


def _ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------------------ class tables
def test_class_tables_agree_field_by_field():
    from voxelnet_amd.targets import CLASS_CFG
    assert set(CLASS_CFG) == set(ot.CLASSES) == set(L.CLASS_NAMES)
    for cls in L.CLASS_NAMES:
        a, b = CLASS_CFG[cls], ot.CLASSES[cls]
        for fa, fb in (("x", "x"), ("y", "y"), ("fw", "fw"), ("fh", "fh"), ("l", "l"), ("w", "w"), ("h", "h"), ("z", "z"),
                       ("pos_iou", "pos"), ("neg_iou", "neg")):
            assert a[fa] == b[fb], (cls, fa)
    p, c = ot.CLASSES["Pedestrian"], ot.CLASSES["Cyclist"]
    assert (p["pos"], p["neg"], p["h"], p["w"], p["l"]) == (0.5, 0.35, 1.73, 0.6, 0.8) and (c["w"], c["l"]) == (0.6, 1.76)
    assert R.THRES == {"Car": 0.7, "Pedestrian": 0.5, "Cyclist": 0.5}


def test_grid_sizes_cover_every_workgroup_shape():
    assert [2 * h * w for h, w in L.SLICE_SHAPES] == [2, 64, 130, 256, 270]
    for cls in ("Pedestrian", "Cyclist"):
        assert L.full_grid(cls).shape == (100, 120, 2, 7)          # N = 24,000 = 93 * 256 + 192
        t = L.tiled_grid(cls)
        assert t.shape == (27, 15, 2, 7) and np.array_equal(t[:9], t[9:18]) and np.array_equal(t[:9], t[18:])
        assert np.array_equal(L.slice_grid(cls, (9, 15)), ot.generate_anchors(cls)[66:75, 22:37])
    assert 24000 % L.BLOCK == 192 and 810 > 3 * L.BLOCK


# ---------------------------------------------------------------------------------------------- target cases
@pytest.mark.parametrize("case", L.full_cases(), ids=_ids(L.full_cases()))
def test_full_grid_cases_hold_their_conditions(case):
    s = case.stats()
    print(case.id, s)
    assert s["thr_pos"] >= 1 and s["argmax_only"] >= 1 and s["pos_and_neg"] >= 1 and s["neg_iou"] >= 1
    assert s["no_pos_box"] >= 1          # a box outside the range: its best IoU is <= 0, its idmax -1


def test_full_grid_cases_match_the_table():
    """the figures the cases were chosen by (box draws in the documented order)"""
    got = {c.id: c.stats() for c in L.full_cases()}
    want = {"Pedestrian-full-seed1-B3": (89, 3, 3, 34), "Pedestrian-full-seed3-B2": (38, 17, 16, 114),
            "Cyclist-full-seed1-B3": (178, 3, 2, 32), "Cyclist-full-seed3-B2": (68, 20, 20, 109)}
    for k, v in want.items():
        assert (got[k]["thr_pos"], got[k]["argmax_only"], got[k]["pos_and_neg"], got[k]["no_pos_box"]) == v, k
    big = [np.abs(i[np.isfinite(i)]).max() for c in L.full_cases() for i in c.iou if i.size]
    assert max(big) > 50          # the union nearly cancels somewhere: IoUs far above 1


def test_structural_conditions():
    cases = L.all_target_cases()
    assert any(0 in c.counts and max(c.counts) > 0 for c in L.full_cases())          # an empty sample beside full ones
    assert any(0 in c.counts and max(c.counts) > 0 for c in L.slice_cases() + L.tiled_cases())
    assert any(128 in c.counts for c in L.full_cases())                              # exactly VN_TARGETS_MAX_GT boxes
    assert all(max(c.counts) == 0 for c in L.empty_cases()) and len(L.empty_cases()) >= 1
    assert {len(c.counts) for c in cases} >= {1, 3}
    for c in cases:
        for b in c.boxes:
            if b.shape[0] >= 3:
                assert np.array_equal(b[0], b[1])          # identical boxes
    for c in L.empty_cases():
        pos, neg, tgt = c.ref
        assert not pos.any() and neg.all() and not tgt.any()


_SLICES = [c for c in L.slice_cases() + L.tiled_cases() if c.cls_name != "Car"]


@pytest.mark.parametrize("case", _SLICES, ids=_ids(_SLICES))
def test_slice_cases_hold_their_conditions(case):
    s = case.stats()
    print(case.id, s)
    if case.n_anchors == 2:          # two anchors: positives is all there is room for
        assert s["thr_pos"] + s["argmax_only"] >= 1
        return
    assert s["thr_pos"] >= 1 and s["argmax_only"] >= 1 and s["pos_and_neg"] >= 1 and s["neg_iou"] >= 1
    if case.grid == "tiled":
        assert s["cross_block_ties"] >= 10


_CAR = [c for c in L.slice_cases() + L.tiled_cases() if c.cls_name == "Car"]


@pytest.mark.parametrize("case", _CAR, ids=_ids(_CAR))
def test_car_slices_hold_arg_max_positives(case):
    """Car at its slice origin: with boxes of 4 m the band where the IoU passes 0.6 lies elsewhere (y near x - 11), so these
    slices hold positives through the arg-max only — every one of them negative as well.  They are here for the partial
    workgroups with Car's constants, not for the IoU regime."""
    s = case.stats()
    assert s["argmax_only"] >= 1 and s["pos_and_neg"] >= 1
    if case.grid == "tiled":
        assert s["cross_block_ties"] >= (10 if len(case.counts) > 1 else 5)


def test_slices_at_the_grid_corner_would_hold_no_positive():
    """the origin matters: the same builder at (0, 0) gives no positive of any kind"""
    for cls in ("Pedestrian", "Cyclist"):
        for seed, counts in L.SLICE_SEEDS:
            anchors = L.slice_grid(cls, (9, 15), origin=(0, 0))
            boxes = L.gt_boxes(cls, seed, counts, L.grid_extent(cls, anchors), L.SLICE_PAD)
            s = L.TargetCase(cls, "corner", seed, counts, anchors, boxes).stats()
            assert s["thr_pos"] == 0 and s["argmax_only"] == 0


_TILED = L.tiled_cases()


@pytest.mark.parametrize("case", _TILED, ids=_ids(_TILED))
def test_tiled_grid_tells_the_tie_rules_apart(case):
    """the oracle's arg-max positives sit in the FIRST copy; an oracle that took the last occurrence answers differently"""
    pos, _, tgt = case.ref
    n1 = case.n_anchors // L.TILES
    c = ot.CLASSES[case.cls_name]
    found = 0
    for b, iou in enumerate(case.iou):
        if iou.shape[1] == 0:
            continue
        thr = (iou > c["pos"]).any(axis=1)
        only = np.flatnonzero((pos[b].reshape(-1) == 1) & ~thr)
        assert (only < n1).all()
        found += len(only)
    assert found >= 1
    wrong = L.last_occurrence_targets(case)
    assert not np.array_equal(wrong[0], pos) and not np.array_equal(wrong[2], tgt)


def test_label_lines_mix_in_other_classes_that_are_dropped():
    for cls in ("Pedestrian", "Cyclist"):
        case = L.target_case(cls, "full", *L.FULL_SEEDS[0])
        labels = [L.label_lines(cls, b, 10 + i) for i, b in enumerate(case.boxes)]
        for lines, b in zip(labels, case.boxes):
            names = [l.split()[0] for l in lines]
            assert names.count(cls) == b.shape[0] and len(set(names) - {cls}) == 5
        got = ot.label_to_gt_box_3d(labels, cls)
        assert [g.shape[0] for g in got] == list(case.counts)
        # the label route's boxes (two decimals) still make positives of both kinds
        pos, neg, _ = ot.generate_targets(labels, case.shape, case.anchors, cls)
        assert pos.sum() >= 1 and (pos * neg).sum() >= 0


def test_car_constants_give_another_answer():
    """what the sensitivity checks rely on: on the Pedestrian full grid Car's thresholds / anchor height change the oracle's
    targets, and Car's anchor height moves the decoded z by more than the decode bar"""
    case = L.target_case("Pedestrian", "full", *L.FULL_SEEDS[0])
    saved = dict(ot.CLASSES["Pedestrian"])
    try:
        ot.CLASSES["Pedestrian"].update(pos=0.6, neg=0.45)
        other = ot.generate_targets_from_boxes(case.boxes, case.shape, case.anchors, "Pedestrian")
    finally:
        ot.CLASSES["Pedestrian"].update(saved)
    assert not np.array_equal(other[0], case.ref[0]) or not np.array_equal(other[1], case.ref[1])
    dc = L.decode_case("Pedestrian", "full", L.DECODE_SEEDS[0])
    for b in range(2):
        idx = D.select(dc.probs[b], op.SCORE_THRES, 64)
        z_ped = D.decode(dc.deltas[b], dc.anchors, idx, "Pedestrian")[:, 2].astype(np.float64)
        z_car = D.decode(dc.deltas[b], dc.anchors, idx, "Car")[:, 2].astype(np.float64)
        bar = 1e-6 + 2.4e-7 * np.abs(z_ped)
        assert (np.abs(z_ped - z_car) > 100 * bar).sum() >= 0.9 * len(idx)


# ---------------------------------------------------------------------------------------------- decode cases
_DEC = L.decode_cases()


@pytest.mark.parametrize("case", _DEC, ids=_ids(_DEC))
def test_clustered_maps_make_the_nms_suppress(case):
    rb, rs = case.ref
    n_cand = case.candidates()
    assert (n_cand > 20).all() and (n_cand <= 96).all()
    for b in range(2):
        # with the reference's constants the walk of detect_ref IS the oracle
        boxes, scores, n_sel, gap = L.reference_walk(case.probs[b], case.deltas[b], case.anchors, case.cls_name,
                                                     op.SCORE_THRES, op.NMS_THRES, op.NMS_POST_TOPK)
        assert np.array_equal(scores, rs[b]) and np.array_equal(boxes, rb[b]), b
        assert n_sel == 20 and 1 <= len(rs[b]) < n_sel          # the reference keeps fewer than it selected
    for st, nt, tk in L.DECODE_PARAMS:
        for b in range(2):
            boxes, scores, n_sel, gap = L.reference_walk(case.probs[b], case.deltas[b], case.anchors, case.cls_name, st, nt, tk)
            print(f"{case.id} sample {b} thres {st} nms {nt} top_k {tk}: selected {n_sel}, kept {len(scores)}, gap {gap:.2e}")
            assert gap > L.NMS_MARGIN, (st, nt, tk, b, gap)
            assert n_sel == min(tk, int((case.probs[b].reshape(-1) >= np.float32(st)).sum()))
            if tk > 1 and (st, nt) == (op.SCORE_THRES, op.NMS_THRES):
                assert len(scores) < n_sel


def test_patches_are_addressed_by_flat_anchor_index():
    """the clustered candidates are neighbouring ANCHORS (cells x 2 rotations): their decoded centres lie within the
    patch, a few metres, which is why the stand-up rectangles overlap"""
    case = L.decode_case("Pedestrian", "full", L.DECODE_SEEDS[0])
    for b in range(2):
        idx = np.flatnonzero(case.probs[b].reshape(-1) >= np.float32(op.SCORE_THRES))
        cells = np.unique(idx // 2)
        assert len(cells) * 2 == len(idx)          # both rotations of every cell
        assert len(idx) <= L.PATCHES * L.PATCH * L.PATCH * 2


# ---------------------------------------------------------------------------------------------- reference helpers
def test_detect_ref_passes_the_class_on():
    case = L.decode_case("Cyclist", (9, 15), L.DECODE_SEEDS[0])
    a = D.detect(case.probs[0], case.deltas[0], case.anchors, 0.96, 20, D.STANDUP, 0.1, 20, cls_name="Cyclist")
    b = D.detect(case.probs[0], case.deltas[0], case.anchors, 0.96, 20, D.STANDUP, 0.1, 20)
    assert np.array_equal(a[1], b[1]) and not np.array_equal(a[0][:, 2], b[0][:, 2])
    assert np.array_equal(a[0], case.ref[0][0])


@pytest.mark.parametrize("cls", ["Pedestrian", "Cyclist"])
def test_class_scenes_drop_the_other_classes(cls):
    scene = R.make_scene(1, n_frames=16, cls_name=cls, others=True)
    c = ot.CLASSES[cls]
    full, own, relabelled = R.RefEvaluator(cls), R.RefEvaluator(cls), R.RefEvaluator(cls)
    n_other = 0
    for det, scores, lines in scene:
        mine = [l for l in lines if l.split()[0] == cls]
        n_other += len(lines) - len(mine)
        assert all(l.split()[0] in R.OTHER_NAMES for l in lines if l.split()[0] != cls)
        full.add_frame(det, scores, lines)
        own.add_frame(det, scores, mine)
        relabelled.add_frame(det, scores, [" ".join([cls] + l.split()[1:]) for l in lines])
        gt, _ = R.frame_ground_truth(lines, cls)
        if len(gt):
            assert (gt[:, 0] > c["x"][0]).all() and (gt[:, 0] < c["x"][1]).all() and (np.abs(gt[:, 1]) < c["y"][1]).all()
            assert np.allclose(gt[:, 4], c["w"], rtol=0.12) and np.allclose(gt[:, 5], c["l"], rtol=0.12)
    assert n_other >= 16
    a, b = full.compute(), own.compute()
    assert a == b and 0 < a["bev"]["all"] < 1 and 0 < a["3d"]["all"] < 1
    assert relabelled.compute() != a          # taken for the class, the mixed-in lines would change the result
    # Car keeps Van as an ignored ground truth; the defaults are the Car scenes as they always were
    assert [l.split()[0] for _, _, ls in R.make_scene(0, n_frames=4) for l in ls].count("Car") > 0
