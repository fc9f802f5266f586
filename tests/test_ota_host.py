"""CPU: the SimOTA reference (tests/ota_ref.py) on the shared cases (tests/ota_cases.py) — the guard that no decision of any
(case, metric, q) lies within ota_cases.MARGIN, asserted ON THE REFERENCE ALONE before tests/test_gpu_ota.py looks at the device
—, properties of the reference's answers, and the part of targets.TargetGenerator's ValueError surface that needs no device."""
import numpy as np
import pytest

import ota_cases as OC
import ota_ref as T

_COMBOS = OC.combos()


def _case(name):
    return next(c for c in OC.cases() if c.id == name)


@pytest.mark.parametrize("combo", _COMBOS, ids=[OC.combo_id(c) for c in _COMBOS])
def test_guard_and_properties(combo):
    case, metric, q = combo
    gaps = case.guard(metric, q)
    print(f"{OC.combo_id(combo)}: smallest gaps {gaps}")
    assert all(g > OC.MARGIN for g in gaps.values())
    for boxes, ref in zip(case.boxes, case.ref(metric, q)):
        st = ref["stats"]
        assert np.array_equal(ref["neg"], ~ref["pos"]) and np.array_equal(ref["pos"], ref["matched"] >= 0)
        for k in range(len(boxes)):
            n_cand = ref["cand"][k].size
            assert st[k, 0] == n_cand
            if n_cand == 0:
                assert not st[k].any() and ref["sel"][k].size == 0
                continue
            assert T.box_valid(boxes[k])
            assert 1 <= st[k, 2] <= min(q, n_cand) and st[k, 2] == ref["sel"][k].size          # dyn_k
            assert st[k, 4] <= st[k, 2]                                                       # won <= dyn_k
            assert len(set(ref["sel"][k].tolist())) == ref["sel"][k].size
            won = np.flatnonzero(ref["matched"] == k)
            assert set(won.tolist()) <= set(ref["sel"][k].tolist())          # no anchor it did not select
        assert st[:, 4].sum() == ref["pos"].sum()                            # no anchor has two boxes


def test_cases_cover_what_they_claim():
    """the special maps and frames do what tests/ota_cases.py says of them"""
    by = {c.id: c for c in OC.cases()}
    assert [len(b) for b in by["Car-5x13"].boxes] == [5, 0, 12]          # the empty middle sample
    extra = by["Car-atss-extra"]
    assert np.array_equal(extra.boxes[0][0], extra.boxes[0][1]) and len(extra.boxes[1]) == 0
    ref = extra.ref("bev", 10)
    assert not (ref[0]["matched"] == 1).any() and (ref[0]["matched"] == 0).any()          # copies: the smaller k takes all
    assert not ref[2]["stats"][0].any() and ref[2]["stats"][1, 0] > 0                     # the invalid box beside a valid one
    assert not ref[3]["stats"].any() and not ref[3]["pos"].any()                          # 30 m off the grid: no candidate
    # radius 0: only in_box anchors, every one with the 1e5 term
    r0 = by["Car-hand-radius0"]
    assert r0.radius == 0.0
    for pairs, ref in zip(r0.pairs(), r0.ref("bev", 10)):
        for pk, cost in zip(pairs, ref["cost"]):
            if pk is not None and pk["n"].size:
                assert not pk["both"].any() and (cost >= T.OUTSIDE).all()
    # the wide radius: every anchor a candidate of both boxes
    wide = by["Car-hand-wide-radius"]
    assert len(wide.boxes) == 8 and len(wide.boxes[1]) == 128 and wide.n_anchors == 1536
    assert [c.size for c in wide.ref("bev", 16)[0]["cand"]] == [1536, 1536] and not wide.ref("bev", 16)[1]["stats"].any()
    # the odd values are candidates inside footprint and radius of box 0, and the overflowing one scores exactly 0
    odd, S = by["Car-hand-odd-values"], by["Car-hand-odd-values"].n_anchors // 2
    p, d = odd.probs[0].reshape(2, S), odd.deltas[0].reshape(14, S)
    pk = odd.pairs()[0][0]
    n_zero, n_nan = (int(np.flatnonzero(m.T.reshape(-1))[0]) for m in (p == 0, np.isnan(p)))
    s200, a200 = (int(x[0]) for x in np.nonzero((d[[3, 10]] == OC.OVERFLOW_D3).T))
    n_200 = 2 * s200 + a200
    cost = dict(zip(pk["n"].tolist(), odd.ref("bev", 10)[0]["cost"][0].tolist()))
    for n in (n_zero, n_nan, n_200):
        assert pk["both"][pk["n"].tolist().index(n)]
    assert pk["v"][pk["n"].tolist().index(n_200)].tolist() == [0.0, 0.0]
    for n in (n_zero, n_nan):
        v = pk["v"][pk["n"].tolist().index(n), 0]
        assert cost[n] == -np.log(1e-12) + 3.0 * -np.log(v + 1e-8) + 0.0
    # zero deltas on the tiled grid: the three copies of an anchor have equal costs
    zero = by["Car-tiled-zero-deltas"]
    ref = zero.ref("bev", 10)[0]
    k = next(k for k in range(len(zero.boxes[0])) if ref["cand"][k].size >= 3)
    n, third = ref["cand"][k], zero.n_anchors // 3
    first = [i for i, x in enumerate(n.tolist()) if x < third and x + third in n.tolist()]
    assert first and all(ref["cost"][k][i] == ref["cost"][k][n.tolist().index(n[i] + third)] for i in first)


def test_scaled_box_takes_the_five_largest_p():
    case = _case("Car-hand-scaled-box")
    assert 7 in case.qs
    for metric in OC.METRICS:
        ref, pk = case.ref(metric, 7)[0], case.pairs()[0][0]
        assert abs(ref["v"][0] - 0.8).max() < 0.005 and pk["both"].sum() >= 5
        assert 5.5 < ref["stats"][0, 1] < 5.7 and ref["stats"][0, 2] == 5
        top = pk["n"][pk["both"]][np.argsort(-pk["p"][pk["both"]])[:5]]
        assert ref["sel"][0].tolist() == top.tolist()
        assert np.array_equal(np.flatnonzero(ref["pos"]), np.sort(top))


def test_raising_p_gets_an_unselected_candidate_selected():
    """a candidate inside footprint and radius that box 0 did not select is selected once its p is raised far enough"""
    case = _case("Car-9x15")
    b, k, q = 0, 0, 10
    ref, pk = case.ref("bev", q)[b], case.pairs()[b][k]
    S, w = case.n_anchors // 2, case.shape[1]
    sel = set(ref["sel"][k].tolist())
    cut = ref["stats"][k, 3]
    # far enough = to 1: a candidate whose IoU term alone stays below the cut cost
    i = next(i for i in ref["order"][k] if pk["both"][i] and int(pk["n"][i]) not in sel
             and T.cost_of(1.0, pk["v"][i, 0], True, case.iou_weight) < cut - OC.MARGIN)
    n = int(pk["n"][i])
    assert pk["p"][i] < 0.99 and ref["cost"][k][i] > cut
    probs = case.probs[b].copy().reshape(2, S)
    probs[n % 2, n // 2] = 1.0
    pairs = T.pair_values(case.anchors, case.boxes[b], probs, case.deltas[b], case.radius)
    again = T.assign_sample(case.anchors, case.boxes[b], pairs, "bev", q, case.iou_weight, case.anchor_h)
    assert n in again["sel"][k].tolist() and again["stats"][k, 2] == ref["stats"][k, 2]          # v did not change: the same dyn_k
    assert set(again["sel"][k].tolist()) - {n} < sel          # it displaced the last one


def test_value_errors_that_need_no_device():
    import torch
    from voxelnet_amd import targets as TG
    a = _case("Car-9x15").anchors
    assert "simota" in TG.ASSIGN_KINDS and TG.OTA_MAX_Q == 16 and sorted(TG.OTA_METRICS) == ["3d", "bev"]
    for kw in (dict(ota_q=0), dict(ota_q=17), dict(ota_q=2.0), dict(ota_q=True), dict(ota_radius=-1.0), dict(ota_radius=float("nan")),
               dict(ota_radius=float("inf")), dict(ota_iou_weight=-0.5), dict(ota_iou_weight=float("nan")),
               dict(ota_iou_weight=float("inf")), dict(ota_iou_weight=None), dict(ota_metric="rotated"), dict(ota_metric=1)):
        for assign in ("simota", "reference"):          # checked always, as atss_top_k is
            with pytest.raises(ValueError):
                TG.TargetGenerator("Car", "cuda:0", anchors=a, assign=assign, **kw)
    with pytest.raises(ValueError):
        TG.site_pitch(a[:1, :1])          # ota_radius=None on a grid of one site
    assert TG.site_pitch(a) == pytest.approx(OC.pitch(a), rel=0, abs=0) and 0.40 < TG.site_pitch(a) < 0.41
    p, d = torch.zeros((2, 2, 9, 15)), torch.zeros((2, 14, 9, 15))
    TG.check_maps("simota", p, d, 2, (9, 15))
    TG.check_maps("atss", None, None, 2, (9, 15))
    for bad in ((None, d), (p, None), (None, None), (p[:1], d), (p, d[:, :7]), (p, torch.zeros((2, 14, 15, 9))), (p.double(), d),
                (p.numpy(), d)):
        with pytest.raises(ValueError):
            TG.check_maps("simota", bad[0], bad[1], 2, (9, 15))
    for other in ("reference", "standup", "rotated", "atss"):
        for bad in ((p, d), (p, None), (None, d)):
            with pytest.raises(ValueError):
                TG.check_maps(other, bad[0], bad[1], 2, (9, 15))
