"""CPU: the host side of the focal / sine-yaw loss objective (vnLossSpec) — the ABI additions, the ctypes
mirror, the argument checks that run before any launch, the reference the GPU tests compare with (tests/focal_ref.py)
against two limits it must reproduce, and a model pickled before the attributes existed."""
import ctypes
import os
import pickle
import subprocess

import pytest
import torch

import focal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vn_rpn_loss_spec_check", "vn_rpn_loss_spec_fwd", "vn_rpn_loss_spec_bwd", "vn_rpn_loss_spec_fwd_bwd",
       "vn_rpn_loss_spec_fwd_bwd_rows")


def _case(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    prob = (torch.rand((B, 2, H, W), generator=g) * 0.98 + 0.01).double()
    delta = (torch.randn((B, 14, H, W), generator=g) * 0.2).double()
    pos = (torch.rand((B, H, W, 2), generator=g) < 0.2).double()
    neg = (torch.rand((B, H, W, 2), generator=g) < 0.8).double() * (1 - pos)
    tgt = (torch.randn((B, H, W, 14), generator=g) * 0.2).double()
    return prob, delta, pos, neg, tgt


def test_abi_version_stays_and_the_new_symbols_are_exported():
    from voxelnet_amd import _lib
    lib = _lib.load()
    assert lib.vn_abi_version() == _lib.ABI_VERSION == 4
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert _lib.missing_symbols() == []


def test_loss_spec_and_step_layouts_equal_the_headers(tmp_path):
    """gcc on include/voxelnet_hip.h, as tests/test_abi.py does for the other structs: sizes and every field offset; the spec
    is the LAST member of vnStep, so a caller that zeroes a vnStep of this size gets the reference's objective"""
    from voxelnet_amd import _lib
    pairs = [("vnLossSpec", _lib.VnLossSpec), ("vnStep", _lib.VnStep)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "voxelnet_hip.h"', 'int main(void) {']
    for cname, st in pairs:
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for fname, _ in st._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {fname}));')
        lines.append('  printf("\\n");')
    lines += ['  printf("%d %d\\n", VN_LOSS_BCE, VN_LOSS_FOCAL);', '  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line, (cname, st) in zip(out, pairs):
        parts = line.split()
        assert parts[0] == cname
        got = [ctypes.sizeof(st)] + [getattr(st, f).offset for f, _ in st._fields_]
        assert got == [int(v) for v in parts[1:]], (cname, got, parts)
    assert out[2].split() == [str(_lib.VN_LOSS_BCE), str(_lib.VN_LOSS_FOCAL)] == ["0", "1"]
    assert ctypes.sizeof(_lib.VnLossSpec) == 16 and _lib.VnStep._fields_[-1][0] == "loss_spec"
    assert bytes(_lib.VnLossSpec()) == bytes(16)                      # the default-constructed mirror is the zeroed spec


def test_spec_check_accepts_and_refuses_on_the_host():
    from voxelnet_amd import _lib
    lib = _lib.load()
    ok = lambda *a: lib.vn_rpn_loss_spec_check(ctypes.byref(_lib.VnLossSpec(*a)))      # noqa: E731
    assert lib.vn_rpn_loss_spec_check(None) == 0 and ok(0, 0, 0.0, 0.0) == 0
    for gamma in (0.0, 1.0, 2.0, 2.5, 5.0):
        for fa in (0.0, 0.25, 1.0):
            assert ok(1, 0, fa, gamma) == 0 and ok(1, 1, fa, gamma) == 0
    for gamma in (-1.0, 0.5, 0.999, float("nan"), float("inf")):
        assert ok(1, 0, 0.25, gamma) == -1, gamma
    for fa in (-0.01, 1.01, float("nan")):
        assert ok(1, 0, fa, 2.0) == -1, fa
    assert ok(2, 0, 0.25, 2.0) == -1 and ok(0, 2, 0.0, 0.0) == -1 and ok(-1, 0, 0.0, 0.0) == -1
    assert ok(0, 1, 7.0, 0.5) == 0                # the focal fields are not read with the reference's classification term
    # the entry points refuse a bad spec before they look at (or launch) anything else; NULL buffers are refused as before
    bad = ctypes.byref(_lib.VnLossSpec(1, 0, 0.25, 0.5))
    one = ctypes.c_void_p(16)                    # never dereferenced: the call returns at the spec
    assert lib.vn_rpn_loss_spec_fwd(one, one, one, one, one, 2, 8, 8, 1.5, 1.0, 3.0, one, 1 << 20, one, None, bad) == -1
    assert lib.vn_rpn_loss_spec_fwd_bwd_rows(None, None, None, None, None, 2, 8, 8, 1.5, 1.0, 3.0, None, 0, None, None, None, None,
                                             1, 16, 0, None, None) == -1


def test_bad_gamma_and_alpha_raise_from_the_host_wrapper():
    from voxelnet_amd import model as M
    for kw in ({"focal_gamma": 0.5}, {"focal_gamma": -1.0}, {"focal_gamma": float("nan")}, {"focal_alpha": 1.5},
               {"focal_alpha": -0.1}):
        with pytest.raises(ValueError):
            M.loss_spec("focal", **{"focal_alpha": 0.25, "focal_gamma": 2.0, **kw})
        with pytest.raises(ValueError):
            M.RPN3D("Car", cls_loss="focal", **kw)
    with pytest.raises(ValueError):
        M.RPN3D("Car", cls_loss="hinge")
    with pytest.raises(ValueError):
        M.RPN3D("Car", yaw_loss="cos")
    m = M.RPN3D("Car", cls_loss="focal", yaw_loss="sin")
    s = m._loss_spec()
    assert (s.cls_kind, s.yaw_sin, s.focal_alpha, s.focal_gamma) == (1, 1, 0.25, 2.0)
    m.focal_gamma = 0.3                          # set after construction: refused at the step, before any launch
    with pytest.raises(ValueError):
        m.loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 14, 4, 4), torch.zeros(1, 4, 4, 2), torch.zeros(1, 4, 4, 2),
               torch.zeros(1, 4, 4, 14))
    with pytest.raises(ValueError):
        m.train_step((None, None, [], None, [], None, None), "cpu")
    d = M.RPN3D("Car")._loss_spec()
    assert bytes(d) == bytes(16)                 # the defaults are the zeroed spec


def test_focal_ref_with_gamma_zero_is_half_a_cross_entropy_over_the_positives_count():
    prob, delta, pos, neg, tgt = _case(3, 6, 5, 1)
    pos[2] = 0                                   # P_b clamps to 1
    got = focal_ref.loss(prob, delta, pos, neg, tgt, 1.5, 1.0, 3.0, cls="focal", fa=0.5, gamma=0.0)
    p_b = pos.sum(dim=(1, 2, 3)).clamp(min=1).reshape(-1, 1, 1, 1)
    ce_pos = (-pos.permute(0, 3, 1, 2) * torch.log(prob + 1e-6) / p_b).sum()
    ce_neg = (-neg.permute(0, 3, 1, 2) * torch.log(1 - prob + 1e-6) / p_b).sum()
    assert torch.allclose(got[3], 0.5 * ce_pos, rtol=1e-12) and torch.allclose(got[4], 0.5 * ce_neg, rtol=1e-12)
    assert torch.allclose(got[1], 0.5 * (1.5 * ce_pos + ce_neg), rtol=1e-12)
    # the regression term is the oracle's, and "bce" is the oracle's loss altogether
    from oracle import torch_ref as tr
    want = tr.rpn_loss(prob, delta, pos, neg, tgt, 1.5, 1.0, 3.0)
    assert torch.allclose(got[2], want[2], rtol=1e-12)
    bce = focal_ref.loss(prob, delta, pos, neg, tgt, 1.5, 1.0, 3.0, cls="bce")
    assert all(torch.allclose(a, b, rtol=1e-12) for a, b in zip(bce, want))


def test_focal_ref_sine_yaw_equals_the_difference_to_first_order():
    """|delta_6 - tgt_6| <= 1e-4: sin(x) = x (1 - x^2/6 + ...), so the two regression sums — and their gradients, through
    cos(x) = 1 - x^2/2 — agree to a relative 1e-8 (x^2 = 1e-8); the other channels are identical"""
    prob, delta, pos, neg, tgt = _case(2, 6, 5, 2)
    g = torch.Generator().manual_seed(5)
    for a in range(2):
        delta[:, a * 7 + 6] = tgt[..., a * 7 + 6] + (torch.rand((2, 6, 5), generator=g).double() * 2 - 1) * 1e-4
    outs = {}
    for yaw in ("diff", "sin"):
        d = delta.clone().requires_grad_(True)
        o = focal_ref.loss(prob, d, pos, neg, tgt, cls="focal", yaw=yaw)
        o[0].backward()
        outs[yaw] = (o, d.grad)
    (od, gd), (os_, gs) = outs["diff"], outs["sin"]
    assert abs(od[2].item() - os_[2].item()) <= 1e-8 * abs(od[2].item())
    assert float((gd - gs).abs().max()) <= 2e-8 * float(gd[:, [6, 13]].abs().max())
    assert all(a.item() == b.item() for a, b in zip(od[3:], os_[3:]))
    # ... and away from the linear range it is another loss: a yaw error of pi costs nothing, one of pi / 2 the most
    for a in range(2):
        delta[:, a * 7 + 6] = tgt[..., a * 7 + 6] + torch.pi
    far = [focal_ref.loss(prob, delta, pos, neg, tgt, cls="focal", yaw=yaw)[2].item() for yaw in ("diff", "sin")]
    for a in range(2):
        delta[:, a * 7 + 6] = tgt[..., a * 7 + 6]
    zero = focal_ref.loss(prob, delta, pos, neg, tgt, cls="focal", yaw="diff")[2].item()
    assert abs(far[1] - zero) <= 1e-12 * zero and far[0] > zero + 1.0


def test_a_model_pickled_without_the_new_attributes_loads_as_bce():
    from voxelnet_amd import model as M
    m = M.RPN3D("Car")
    state = m.__getstate__()
    for k in ("cls_loss", "focal_alpha", "focal_gamma", "yaw_loss"):
        assert k in state
        del state[k]                             # what a checkpoint written before this change holds
    old = M.RPN3D.__new__(M.RPN3D)
    old.__setstate__(pickle.loads(pickle.dumps(state)))
    assert "cls_loss" not in old.__dict__
    assert (old.cls_loss, old.focal_alpha, old.focal_gamma, old.yaw_loss) == ("bce", 0.25, 2.0, "diff")
    assert bytes(old._loss_spec()) == bytes(16)
    # and a focal model keeps its objective through a round trip
    f = pickle.loads(pickle.dumps(M.RPN3D("Car", cls_loss="focal", focal_gamma=1.0, yaw_loss="sin")))
    assert (f.cls_loss, f.focal_gamma, f.yaw_loss) == ("focal", 1.0, "sin")
