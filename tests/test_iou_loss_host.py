"""CPU: the host side of the rotated-IoU regression loss — the reference the GPU tests compare with
(tests/iou_loss_ref.py) against the scoring reference (tests/eval_ref.py) and against central differences of it, the DIoU
term against a NumPy restatement, the ABI additions and their ctypes mirror, the argument checks that run before any
launch, the module's argument checks, and the structs the entry point must leave alone."""
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import eval_ref
import iou_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vn_rpn_iou_loss_workspace_bytes", "vn_rpn_iou_loss")
SHAPE = (2, 17, 15)          # ~100 positives: a second for the loops below
K = {"bev": 0, "3d": 1}


def _decode_np(d, A):
    """the decode in NumPy float64 — a restatement of its own, not iou_loss_ref's"""
    d = np.asarray(d, dtype=np.float64)
    diag = math.sqrt(A[4] ** 2 + A[5] ** 2)
    return np.array([d[0] * diag + A[0], d[1] * diag + A[1], d[2] * A[3] + A[2], math.exp(d[3]) * A[3], math.exp(d[4]) * A[4],
                     math.exp(d[5]) * A[5], d[6] + A[6]])


@functools.lru_cache(maxsize=None)
def _generic():
    B, H, W = SHAPE
    delta, pos, tgt = R.generic_inputs(B, H, W, 11)
    return delta, pos, tgt, R.small_anchors(H, W)


@pytest.mark.parametrize("metric", ["bev", "3d"])
def test_reference_equals_eval_ref_and_its_central_differences(metric):
    """values at 1e-12; autograd at 1e-6 of the gradient's maximum against central differences (h = 1e-6) of
    eval_ref.iou_pair through the NumPy decode.  Every generic pair overlaps: none is left out."""
    delta, pos, tgt, anchors = _generic()
    B, H, W = SHAPE
    d64 = delta.double().requires_grad_(True)
    loss, mean_iou, pairs = R.loss(d64, pos, tgt, anchors, "iou", metric)
    # the sum of the pairs' IoUs, so that autograd hands back every pair's own derivative
    (-loss).backward()          # loss = sum (1 - IoU) / P_b: d(-loss) / d delta = dIoU / P_b
    p_b = pos.sum(dim=(1, 2, 3)).clamp(min=1.0)
    assert len(pairs) == int(pos.sum()) > 50
    worst_v, worst_g, gmax = 0.0, 0.0, 0.0
    h = 1e-6
    for (b, y, x, a), iou, L in pairs:
        A = anchors[y, x, a]
        d = delta[b, a * 7:a * 7 + 7, y, x].double().numpy()
        G = _decode_np(tgt[b, y, x, a * 7:a * 7 + 7].double().numpy(), A)
        want = eval_ref.iou_pair(_decode_np(d, A), G)[K[metric]]
        assert want > 0.0, (b, y, x, a)
        worst_v = max(worst_v, abs(iou - want), abs(L - (1.0 - want)))
        got = d64.grad[b, a * 7:a * 7 + 7, y, x].numpy() * float(p_b[b])
        for j in range(7):
            e = np.zeros(7)
            e[j] = h
            cd = (eval_ref.iou_pair(_decode_np(d + e, A), G)[K[metric]] - eval_ref.iou_pair(_decode_np(d - e, A), G)[K[metric]]) / (2 * h)
            worst_g = max(worst_g, abs(got[j] - cd))
            gmax = max(gmax, abs(cd))
    print(f"{metric}: values {worst_v:.1e}, gradient {worst_g / gmax:.1e} of its maximum {gmax:.3f}")
    assert worst_v <= 1e-12
    assert gmax > 0 and worst_g <= 1e-6 * gmax
    want_mean = np.mean([p[1] for p in pairs])
    assert abs(float(mean_iou) - want_mean) <= 1e-12
    assert d64.grad[pos.repeat_interleave(7, dim=3).permute(0, 3, 1, 2) == 0].abs().max().item() == 0.0


def _corners_np(box):
    x, y, _, _, w, l, r = box
    c, s = math.cos(r), math.sin(r)
    return np.array([[x + u * c - v * s, y + u * s + v * c] for u, v in ((l / 2, w / 2), (-l / 2, w / 2), (-l / 2, -w / 2), (l / 2, -w / 2))])


@pytest.mark.parametrize("metric", ["bev", "3d"])
def test_diou_adds_the_distance_term(metric):
    delta, pos, tgt, anchors = _generic()
    _, _, plain = R.loss(delta, pos, tgt, anchors, "iou", metric)
    _, _, diou = R.loss(delta, pos, tgt, anchors, "diou", metric)
    worst = 0.0
    for ((b, y, x, a), iou0, L0), (idx, iou1, L1) in zip(plain, diou):
        assert idx == (b, y, x, a) and iou0 == iou1
        A = anchors[y, x, a]
        P = _decode_np(delta[b, a * 7:a * 7 + 7, y, x].double().numpy(), A)
        G = _decode_np(tgt[b, y, x, a * 7:a * 7 + 7].double().numpy(), A)
        pts = np.concatenate([_corners_np(P), _corners_np(G)])
        ext = pts.max(axis=0) - pts.min(axis=0)
        rho2, c2 = (G[0] - P[0]) ** 2 + (G[1] - P[1]) ** 2, ext[0] ** 2 + ext[1] ** 2
        if metric == "3d":
            rho2 += ((G[2] + G[3] / 2) - (P[2] + P[3] / 2)) ** 2
            c2 += (max(P[2] + P[3], G[2] + G[3]) - min(P[2], G[2])) ** 2
        assert rho2 / c2 > 0
        worst = max(worst, abs((L1 - L0) - rho2 / c2))
    assert worst <= 1e-12, worst


def test_reference_edge_rules():
    """invalid pairs are the constants (0, 1) without a gradient; disjoint boxes have gradient 0 in "iou" and a
    gradient in "diou"; a yaw turned by pi gives the same IoU"""
    A = torch.tensor([10.0, 5.0, -1.0, 1.56, 1.6, 3.9, 0.0], dtype=torch.float64)
    g = torch.tensor([0.05, -0.02, 0.01, 0.02, -0.03, 0.04, 0.1], dtype=torch.float64)
    G = R.decode(g, A)
    for bad in ([0, 0, 0, math.inf, 0, 0, 0], [math.nan, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1000.0, 0, 0]):
        d = torch.tensor(bad, dtype=torch.float64, requires_grad=True)
        for kind in ("iou", "diou"):
            for metric in ("bev", "3d"):
                iou, L = R.pair_loss(R.decode(d, A), G, kind, metric)
                assert iou.item() == 0.0 and L.item() == 1.0 and not L.requires_grad
    far = torch.tensor([7.0, 0.1, 0.0, 0.1, -0.1, 0.05, 0.3], dtype=torch.float64, requires_grad=True)
    iou, L = R.pair_loss(R.decode(far, A), G, "iou", "3d")
    assert iou.item() == 0.0 and L.item() == 1.0
    assert not L.requires_grad or torch.autograd.grad(L, far)[0].abs().max().item() == 0.0
    iou, L = R.pair_loss(R.decode(far, A), G, "diou", "3d")
    assert iou.item() == 0.0 and L.item() > 1.0 and torch.autograd.grad(L, far)[0].abs().max().item() > 0.0
    near = torch.tensor([0.1, 0.05, 0.02, 0.1, -0.1, 0.05, 0.3], dtype=torch.float64)
    turned = near.clone()
    turned[6] += math.pi
    a, b = R.pair_loss(R.decode(near, A), G, "iou", "3d")[0], R.pair_loss(R.decode(turned, A), G, "iou", "3d")[0]
    assert 0.1 < a.item() < 1.0 and abs(a.item() - b.item()) <= 1e-14


@pytest.mark.parametrize("shape", list(R.SEAM_CASES), ids=lambda s: "x".join(str(v) for v in s))
def test_seam_cases_hold_the_guard(shape):
    """the inputs of tests/test_gpu_iou_loss.py's seam test, on the reference alone: the positives are exactly where
    iou_loss_ref.SEAM_CASES says and reach the loops they are there for; every pair overlaps; the loss is finite and not 0"""
    B, H, W = shape
    flat = R.SEAM_CASES[shape]
    delta, pos, tgt, anchors = R.seam_inputs(shape)
    assert sorted(torch.nonzero(pos.reshape(-1)).reshape(-1).tolist()) == sorted(flat) and float(pos.sum()) == len(flat) <= 12
    sites, per_b, last = B * H * W, H * W * 2, B * H * W * 2 - 1
    assert {0, last} <= set(flat)
    if B == 1:          # the normaliser's second sweep: elements at and beyond 16 x 256, fewer than another full sweep
        assert 16 * 256 < per_b < 2 * 16 * 256 and {16 * 256 - 1, 16 * 256} <= set(flat)
    else:               # a second slab row for finalize thread 0; a workgroup that holds the end of sample 0 and the start of sample 1
        assert (sites + 255) // 256 == 257 and sum(f // 2 >= 256 * 256 for f in flat) >= 2
        assert {2 * (H * W - 1) + 1, 2 * H * W} <= set(flat) and (H * W - 1) // 256 == (H * W) // 256
        p_b = pos.sum(dim=(1, 2, 3)).tolist()
        assert p_b[0] != p_b[1] and min(p_b) >= 1
    for kind, metric in (("iou", "bev"), ("diou", "3d")):
        d64 = delta.double().requires_grad_(True)
        loss, mean_iou, pairs = R.loss(d64, pos, tgt, anchors, kind, metric)
        loss.backward()
        assert len(pairs) == len(flat) and all(p[1] > 0.0 for p in pairs)
        assert math.isfinite(loss.item()) and loss.item() > 0 and 0 < mean_iou.item() < 1
        assert torch.isfinite(d64.grad).all() and d64.grad.abs().max().item() > 0


def test_header_declares_and_lib_binds_the_new_symbols():
    from voxelnet_amd import _lib
    lib = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voxelnet_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", text), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert _lib.missing_symbols() == []
    assert lib.vn_abi_version() == _lib.ABI_VERSION == 4          # additive: the version stays
    for name, val in (("VN_IOU_LOSS_IOU", 0), ("VN_IOU_LOSS_DIOU", 1), ("VN_IOU_BEV", 0), ("VN_IOU_3D", 1)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(val) + r"\b", text), name
        assert getattr(_lib, name) == val
    assert (_lib.VN_IOU_BEV, _lib.VN_IOU_3D) == (_lib.VN_EVAL_BEV, _lib.VN_EVAL_3D)


def test_entry_point_refuses_bad_arguments_before_touching_a_pointer():
    from voxelnet_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)          # never dereferenced: every call below returns at a check
    big = 1 << 24

    def call(B=2, H=8, W=8, kind=0, metric=1, ws_bytes=big, ptr=one):
        return lib.vn_rpn_iou_loss(ptr, ptr, ptr, ptr, B, H, W, kind, metric, None, ptr, ws_bytes, ptr, None, None)
    for kind in (-1, 2, 7):
        assert call(kind=kind) == -1 and call(kind=kind, ptr=None) == -1
    for metric in (-1, 2):
        assert call(metric=metric) == -1 and call(metric=metric, ptr=None) == -1
    for size in ({"B": 0}, {"H": 0}, {"W": -3}, {"B": 1 << 11, "H": 1 << 10, "W": 1 << 10}):
        assert call(**size) == -1
        assert lib.vn_rpn_iou_loss_workspace_bytes(size.get("B", 2), size.get("H", 8), size.get("W", 8)) == 0
    assert call(ptr=None) == -1          # good sizes, NULL buffers
    need = lib.vn_rpn_iou_loss_workspace_bytes(2, 8, 8)
    assert need > 0 and need % 256 == 0
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3          # VN_EWORKSPACE
    # the car map and the dense map: a few KB
    assert 0 < lib.vn_rpn_iou_loss_workspace_bytes(2, 200, 176) < lib.vn_rpn_iou_loss_workspace_bytes(4, 200, 176) < 1 << 16


def test_module_refuses_bad_settings():
    from voxelnet_amd import iou_loss as IL
    from voxelnet_amd import model as M
    with pytest.raises(ValueError):
        M.RPN3D("Car", iou_loss="giou")
    with pytest.raises(ValueError):
        M.RPN3D("Car", iou_loss="iou", iou_metric="2d")
    for w in (float("nan"), float("inf"), "heavy"):
        with pytest.raises(ValueError):
            M.RPN3D("Car", iou_loss="diou", iou_weight=w)
    d = M.RPN3D("Car")
    assert (d.iou_loss, d.iou_weight, d.iou_metric, d.last_iou) == (None, 1.0, "3d", None) and d._iou_spec() is None
    m = M.RPN3D("Car", iou_loss="diou", iou_weight=2.0, iou_metric="bev")
    assert m._iou_spec() == ("diou", "bev", 2.0)
    assert not m._step_fused_ok("bf16", None)          # the term is not part of vn_net_step
    m.iou_metric = "2d"                                # set after construction: refused when read, before any launch
    z = torch.zeros
    with pytest.raises(ValueError):
        m.loss(z(1, 2, 4, 4), z(1, 14, 4, 4), z(1, 4, 4, 2), z(1, 4, 4, 2), z(1, 4, 4, 14))
    with pytest.raises(ValueError):
        m.train_step((None, None, [], None, [], None, None), "cpu")
    with pytest.raises(ValueError):
        IL.rpn_iou_loss(z(1, 14, 4, 4), z(1, 4, 4, 2), z(1, 4, 4, 14), z(32, 7, dtype=torch.float64), kind="giou")
    with pytest.raises(_lib_error()):                   # no CPU path
        IL.rpn_iou_loss(z(1, 14, 4, 4), z(1, 4, 4, 2), z(1, 4, 4, 14), z(32, 7, dtype=torch.float64))


def _lib_error():
    from voxelnet_amd import _lib
    return _lib.VoxelnetHipError


def test_loss_spec_and_step_are_unchanged(tmp_path):
    """the entry point is additive: vnLossSpec keeps its 16 bytes, vnStep its 552 and loss_spec as its last member"""
    from voxelnet_amd import _lib
    src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "voxelnet_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(vnLossSpec), sizeof(vnStep), offsetof(vnStep, loss_spec)); return 0; }\n')
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out] == [16, 552, 536]
    assert ctypes.sizeof(_lib.VnLossSpec) == 16 and ctypes.sizeof(_lib.VnStep) == 552
    assert _lib.VnStep._fields_[-1][0] == "loss_spec" and _lib.VnStep.loss_spec.offset == 536 and len(_lib.VnStep._fields_) == 54
