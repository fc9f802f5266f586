"""CPU: the inputs of the ATSS tests (tests/atss_cases.py) keep their guard ON THE REFERENCE ALONE (tests/atss_ref.py) — no
decision of any (case, kind, top_k) tests/test_gpu_atss.py runs lies within MARGIN = 1e-7 — and the reference has the
properties the rules promise.  Nothing here touches the library's kernels."""
import numpy as np
import pytest

import atss_cases as AC
import atss_ref as T

_COMBOS = AC.combos()


@pytest.mark.parametrize("combo", _COMBOS, ids=[AC.combo_id(c) for c in _COMBOS])
def test_guard_and_properties(combo):
    case, kind, top_k = combo
    gaps = case.guard(kind, top_k)
    print(f"{AC.combo_id(combo)}: smallest gaps {gaps}")
    assert all(g > AC.MARGIN for g in gaps.values())
    a = case.anchors.reshape(-1, 7)
    N, K = a.shape[0], min(top_k, a.shape[0] // 2)
    for boxes, s in zip(case.boxes, case.ref(kind, top_k)):
        assert np.array_equal(s["pos"], ~s["neg"]) and np.array_equal(s["pos"], s["matched"] >= 0)          # a partition
        assert s["stats"][:, 3].sum() == s["pos"].sum()
        if len(boxes) == 0:
            assert s["neg"].all() and s["stats"].shape == (0, 4)
        for k, q in enumerate(boxes):
            c, v, t = s["cand"][k], s["v"][k], s["stats"][k, 2]
            if not T.box_valid(q):
                assert c.size == 0 and not s["stats"][k].any() and not (s["matched"] == k).any()
                continue
            assert c.size == 2 * K >= 2 and np.unique(c).size == c.size
            assert (c[:K] % 2 == 0).all() and (c[K:] % 2 == 1).all()
            if top_k >= N // 2:
                assert np.array_equal(np.sort(c), np.arange(N))          # every anchor is a candidate
            for n in np.flatnonzero(s["matched"] == k):          # a positive: a candidate at or above t with its centre inside
                i = int(np.flatnonzero(c == n)[0])
                assert v[i] >= t and v[i] > 0 and max(T.local_offsets(a[n], q)) <= 0
            assert not (s["targets"][s["neg"]] != 0).any()


def test_what_the_extra_frames_hold():
    case = next(c for c in AC.cases() if c.id == "Car-atss-extra")
    for kind in AC.KINDS:
        copies, empty, invalid, off = case.ref(kind, 9)
        assert copies["pos"].sum() >= 3 and (copies["matched"][copies["pos"]] == 0).all()          # the smaller k takes all
        assert copies["stats"][0, 3] == copies["pos"].sum() and copies["stats"][1, 3] == 0
        assert np.array_equal(copies["stats"][0, :3], copies["stats"][1, :3])
        assert empty["neg"].all()
        assert not invalid["stats"][0].any() and invalid["stats"][1, 3] == invalid["pos"].sum() >= 3
        assert off["cand"][0].size == 18 and not off["v"][0].any() and not off["stats"].any() and off["neg"].all()


def test_the_small_grid_makes_every_anchor_a_candidate():
    case = next(c for c in AC.cases() if c.id == "Car-4x7-one-box")
    assert case.n_anchors == 56 and len(case.boxes) == 1 and len(case.boxes[0]) == 1
    s = case.ref("rotated", 32)[0]
    assert np.array_equal(np.sort(s["cand"][0]), np.arange(56)) and s["pos"].sum() >= 3


def test_ranking_breaks_ties_by_the_smaller_index():
    """two anchors at the same distance from a box (mirror images across it) rank by n, and a repeated anchor row likewise"""
    a = np.zeros((3, 1, 2, 7))
    a[..., 3:6] = (1.56, 1.6, 3.9)
    a[:, 0, :, 0] = np.array([1.0, 3.0, 1.0])[:, None]          # sites 0 and 2 coincide; site 1 mirrors them across x = 2
    a[..., 1, 6] = np.pi / 2
    groups, d2 = T.ranked(a, np.array([2.0, 0.0, -1.0, 1.5, 1.6, 3.9, 0.0]))
    assert d2[0] == d2[2] == d2[4] and list(groups[0]) == [0, 2, 4] and list(groups[1]) == [1, 3, 5]
