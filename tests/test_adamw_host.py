"""CPU: the host side of the fused gradient-clip + AdamW tail (vn_clip_adamw, csrc/optim.hip; voxelnet_amd.optim.ClipAdamW):
the symbols and the ctypes mirror of the header, the argument checks (status codes, before any HIP call — there is no device
here), the optimizer's torch.optim.Optimizer face and its state-dict exchange with torch.optim.AdamW, and
decay_param_groups on the detector's real tensor set.  The arithmetic is tested on the GPU (tests/test_gpu_adamw.py)."""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "voxelnet_hip.h")
NAMES = ("vn_clip_adamw_workspace_bytes", "vn_clip_adamw")


def test_header_library_and_binding_agree_on_the_symbols():
    from voxelnet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} is not declared in the header"
        assert hasattr(lib, n), f"{n} is not exported by the library"
        assert n in _lib.SIGNATURES
    assert re.search(r"#define\s+VN_OPT_MAX_SLOTS\s+8\b", text) and _lib.VN_OPT_MAX_SLOTS == 8
    assert lib.vn_abi_version() == 4          # additive: no signature, layout or protocol of the existing ABI moved


def test_adam_structures_match_the_header_layout(tmp_path):
    """sizes and field offsets of the three structs as gcc lays the header out (the method of
    test_abi.test_ctypes_structures_match_the_header_layout)"""
    from voxelnet_amd import _lib
    pairs = [("vnAdamChunk", _lib.VnAdamChunk), ("vnAdamSlot", _lib.VnAdamSlot), ("vnAdamHyper", _lib.VnAdamHyper)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "voxelnet_hip.h"', 'int main(void) {']
    for cname, st in pairs:
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for fname, _ in st._fields_:
            lines.append(f'  printf(" %zu", offsetof({cname}, {fname}));')
        lines.append('  printf("\\n");')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(out) == len(pairs)
    for line, (cname, st) in zip(out, pairs):
        parts = line.split()
        assert parts[0] == cname
        assert [ctypes.sizeof(st)] + [getattr(st, f).offset for f, _ in st._fields_] == [int(v) for v in parts[1:]], cname
    assert ctypes.sizeof(_lib.VnAdamChunk) == 40 and ctypes.sizeof(_lib.VnAdamSlot) == 24
    assert ctypes.sizeof(_lib.VnAdamHyper) == 4 + 8 * 24


def _hyper(_lib, n_slots=1, **kw):
    h = _lib.VnAdamHyper()
    h.n_slots = n_slots
    for k in range(_lib.VN_OPT_MAX_SLOTS):
        s = h.slot[k]
        s.lr, s.beta1, s.beta2, s.eps, s.weight_decay, s.step = 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1
    for name, value in kw.items():
        setattr(h.slot[n_slots - 1 if 1 <= n_slots <= 8 else 0], name, value)
    return h


def test_argument_checks_return_status_codes():
    """every check of the header's list, with no device: the pointers are never followed (a call that got past the checks
    would reach the HIP runtime and return a positive hipError_t, not -1 / -3)"""
    from voxelnet_amd import _lib
    lib = _lib.load()
    EINVAL, EWORKSPACE = -1, -3
    assert lib.vn_clip_adamw_workspace_bytes(0) == 0 and lib.vn_clip_adamw_workspace_bytes(-3) == 0
    assert lib.vn_clip_adamw_workspace_bytes(1) >= 4
    need = lib.vn_clip_adamw_workspace_bytes(1663)
    assert need >= 4 * 1663
    table = (_lib.VnAdamChunk * 4)()           # host memory standing in for the device pointers: never dereferenced
    ws = (ctypes.c_char * 64)()
    tab, wsp = ctypes.addressof(table), ctypes.addressof(ws)
    nan = float("nan")

    def call(chunks=tab, n_chunks=1663, hyper=None, max_norm=5.0, ws_ptr=wsp, ws_bytes=need - 1, null_hyper=False):
        h = None if null_hyper else ctypes.byref(hyper if hyper is not None else _hyper(_lib))
        return lib.vn_clip_adamw(chunks, n_chunks, h, max_norm, 0, ws_ptr, ws_bytes, None, None)

    # all arguments good except a workspace one byte short: the last check before the launches
    assert call() == EWORKSPACE
    assert call(ws_bytes=0) == EWORKSPACE
    assert call(hyper=_hyper(_lib, 8)) == EWORKSPACE and call(hyper=_hyper(_lib, 3, step=7)) == EWORKSPACE
    assert call(hyper=_hyper(_lib, beta1=0.0, beta2=0.0, eps=0.0, lr=0.0, weight_decay=0.0)) == EWORKSPACE     # the closed ends
    assert call(max_norm=float("inf")) == EWORKSPACE
    # NULL pointers
    assert call(chunks=None) == EINVAL
    assert call(null_hyper=True) == EINVAL
    assert call(ws_ptr=None) == EINVAL
    # sizes
    for n in (0, -1):
        assert call(n_chunks=n) == EINVAL
    for mn in (0.0, -5.0, nan):
        assert call(max_norm=mn) == EINVAL
    for ns in (0, -1, 9, 1 << 20):
        assert call(hyper=_hyper(_lib, ns)) == EINVAL
    # slots: each field on its own, in the first and in the last of several slots
    bad = [("beta1", 1.0), ("beta1", -0.1), ("beta1", nan), ("beta2", 1.0), ("beta2", 1.5), ("beta2", -1e-3), ("beta2", nan),
           ("eps", -1e-8), ("eps", nan), ("lr", -1e-3), ("lr", nan), ("weight_decay", -0.01), ("weight_decay", nan),
           ("step", 0), ("step", -4)]
    for name, value in bad:
        assert call(hyper=_hyper(_lib, 1, **{name: value})) == EINVAL, (name, value)
        assert call(hyper=_hyper(_lib, 5, **{name: value})) == EINVAL, (name, value, "slot 4 of 5")
    # a bad value beyond n_slots is not looked at
    h = _hyper(_lib, 2)
    h.slot[2].beta1 = 2.0
    assert call(hyper=h) == EWORKSPACE


def _params(n=3):
    g = torch.Generator().manual_seed(1)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in [(4, 3), (5,), (2, 2, 2)][:n]]


def test_clip_adamw_is_a_torch_optimizer_without_a_cpu_path():
    from voxelnet_amd import _lib
    from voxelnet_amd.optim import ClipAdamW
    ps = _params()
    opt = ClipAdamW(ps, lr=2e-3, weight_decay=0.05, max_norm=5.0)
    assert isinstance(opt, torch.optim.Optimizer)
    assert opt.defaults["betas"] == (0.9, 0.999) and opt.defaults["eps"] == 1e-8 and opt.defaults["max_norm"] == 5.0
    assert opt.defaults["scale_grads"] is False and opt.param_groups[0]["lr"] == 2e-3
    # schedulers attach: OneCycleLR finds `betas` in defaults (cycle_momentum) and writes lr / betas into the groups
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-2, total_steps=6, pct_start=0.5, cycle_momentum=True)
    assert opt.param_groups[0]["betas"] == (0.95, 0.999) and opt.param_groups[0]["lr"] == pytest.approx(1e-2 / 25)
    assert sched.get_last_lr() == [opt.param_groups[0]["lr"]]
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(_lib.VoxelnetHipError):
        opt.step()
    with pytest.raises(_lib.VoxelnetHipError):
        opt.step(closure=lambda: 0.0)
    assert all(len(opt.state.get(p, {})) == 0 for p in ps)          # nothing was allocated or touched
    opt.zero_grad()
    assert all(p.grad is None for p in ps) and opt.step() is None
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(eps=-1.0), dict(weight_decay=-1.0),
               dict(max_norm=0.0)):
        with pytest.raises(ValueError):
            ClipAdamW(_params(), **kw)
    with pytest.raises(ValueError):
        ClipAdamW([])
    # max_norm / scale_grads are global: groups that disagree raise at step()
    two = ClipAdamW([{"params": ps[:1]}, {"params": ps[1:], "max_norm": 1.0}])
    ps[0].grad = torch.ones_like(ps[0])
    with pytest.raises(_lib.VoxelnetHipError, match="max_norm"):
        two.step()


def test_state_dicts_travel_between_clip_adamw_and_torch_adamw():
    from voxelnet_amd.optim import ClipAdamW
    ps = _params()
    groups = lambda q: [{"params": q[:2], "weight_decay": 0.01, "lr": 2e-3}, {"params": q[2:], "weight_decay": 0.0}]  # noqa: E731
    ref = torch.optim.AdamW(groups(ps), betas=(0.85, 0.99), eps=1e-7)
    for _ in range(2):
        for p in ps:
            p.grad = torch.full_like(p, 0.5)
        ref.step()
    sd = copy.deepcopy(ref.state_dict())
    # torch -> ours: state and hyperparameters arrive, max_norm / scale_grads come from OUR defaults
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    ours = ClipAdamW(groups(qs), max_norm=3.0, scale_grads=True)
    ours._table = object()                                           # (stands for a built device table)
    ours.load_state_dict(sd)
    assert ours._table is None                                       # rebuilt on the next step
    for g, want in zip(ours.param_groups, sd["param_groups"]):
        assert g["betas"] == (0.85, 0.99) and g["eps"] == 1e-7 and g["lr"] == want["lr"] and g["weight_decay"] == want["weight_decay"]
        assert g["max_norm"] == 3.0 and g["scale_grads"] is True
    for q, p in zip(qs, ps):
        st = ours.state[q]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and float(st["step"]) == 2.0
        assert torch.equal(st["exp_avg"], ref.state[p]["exp_avg"]) and torch.equal(st["exp_avg_sq"], ref.state[p]["exp_avg_sq"])
    # ours -> torch: the extra group keys ride along and torch steps on
    back = torch.optim.AdamW(groups([torch.nn.Parameter(p.detach().clone()) for p in ps]))
    back.load_state_dict(copy.deepcopy(ours.state_dict()))
    assert back.param_groups[0]["max_norm"] == 3.0 and back.param_groups[0]["betas"] == (0.85, 0.99)
    for p in ps:
        p.grad = torch.full_like(p, -0.25)
    ref.step()
    bp = [p for g in back.param_groups for p in g["params"]]
    for p in bp:
        p.grad = torch.full_like(p, -0.25)
    back.step()
    for p, q in zip(ps, bp):
        assert torch.equal(p.detach(), q.detach()) and float(back.state[q]["step"]) == 3.0
    # copies and pickles come back without the device-side caches and with the defaults filled in
    import pickle
    for clone in (copy.deepcopy(ours), pickle.loads(pickle.dumps(ours))):
        assert clone._table is None and clone._plist is None
        assert clone.param_groups[1]["max_norm"] == 3.0 and len(clone.state) == 3


def test_decay_param_groups_splits_the_detector():
    from voxelnet_amd import model as M
    from voxelnet_amd.optim import ClipAdamW, decay_param_groups
    m = M.RPN3D("Car")
    groups = decay_param_groups(m, 0.01)
    assert len(groups) == 2 and groups[0]["weight_decay"] == 0.01 and groups[1]["weight_decay"] == 0.0
    allp = list(m.parameters())
    ids = [id(p) for g in groups for p in g["params"]]
    assert len(ids) == len(set(ids)) == len(allp) == 104 and set(ids) == {id(p) for p in allp}
    assert sum(p.numel() for g in groups for p in g["params"]) == 6809392
    assert all(p.dim() > 1 for p in groups[0]["params"]) and all(p.dim() == 1 for p in groups[1]["params"])
    assert {id(p) for p in allp if p.dim() == 1} == {id(p) for p in groups[1]["params"]}
    for mod in m.modules():
        if isinstance(mod, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.BatchNorm3d)):
            assert {id(mod.weight), id(mod.bias)} <= {id(p) for p in groups[1]["params"]}
    opt = ClipAdamW(groups, lr=2e-3)
    assert [g["weight_decay"] for g in opt.param_groups] == [0.01, 0.0] and len(opt.params) == 104
