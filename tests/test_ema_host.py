"""CPU: the host side of the weight average (vn_ema_update, vn_clip_sgd_ema, vn_clip_adamw_ema in csrc/optim.hip;
voxelnet_amd.ema.ModelEMA): the symbols and the ctypes mirror of the header, the argument checks (status codes, before any
HIP call — there is no device here), the decay schedule against its closed forms, and ModelEMA's state on CPU tensors.
The arithmetic is tested on the GPU (tests/test_gpu_ema.py)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import ema_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "voxelnet_hip.h")
NAMES = ("vn_ema_update", "vn_clip_sgd_ema", "vn_clip_adamw_ema")


def test_header_library_and_binding_agree_on_the_symbols():
    from voxelnet_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, text), f"{n} is not declared in the header"
        assert hasattr(lib, n), f"{n} is not exported by the library"
        assert n in _lib.SIGNATURES
    assert lib.vn_abi_version() == 4          # additive: no signature, layout or protocol of the existing ABI moved


def test_ema_structures_match_the_header_layout(tmp_path):
    """sizes and field offsets of the three structs as gcc lays the header out (the method of
    test_abi.test_ctypes_structures_match_the_header_layout)"""
    from voxelnet_amd import _lib
    pairs = [("vnEmaChunk", _lib.VnEmaChunk), ("vnParamChunkEma", _lib.VnParamChunkEma), ("vnAdamChunkEma", _lib.VnAdamChunkEma)]
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
    assert ctypes.sizeof(_lib.VnEmaChunk) == 24 and ctypes.sizeof(_lib.VnParamChunkEma) == 32
    assert ctypes.sizeof(_lib.VnAdamChunkEma) == 48
    # the optimizers' and the average's NumPy rows are these structs
    from voxelnet_amd import ema, optim
    assert ema._EMA_ROW.itemsize == 24 and optim._SGD_EMA_ROW.itemsize == 32 and optim._ADAM_EMA_ROW.itemsize == 48
    for row, st in ((ema._EMA_ROW, _lib.VnEmaChunk), (optim._SGD_EMA_ROW, _lib.VnParamChunkEma),
                    (optim._ADAM_EMA_ROW, _lib.VnAdamChunkEma)):
        assert [(n, row.fields[n][1]) for n in row.names] == [(f, getattr(st, f).offset) for f, _ in st._fields_]


def _hyper(_lib, n_slots=1, **kw):
    h = _lib.VnAdamHyper()
    h.n_slots = n_slots
    for k in range(_lib.VN_OPT_MAX_SLOTS):
        s = h.slot[k]
        s.lr, s.beta1, s.beta2, s.eps, s.weight_decay, s.step = 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1
    for name, value in kw.items():
        setattr(h.slot[n_slots - 1 if 1 <= n_slots <= 8 else 0], name, value)
    return h


EINVAL, EWORKSPACE = -1, -3
NAN = float("nan")
BAD_WEIGHTS = (-0.1, 1.5, NAN)


def test_ema_update_argument_checks():
    """every call here is refused by a check: the table is host memory and must never reach a launch (vn_ema_update has no
    workspace argument whose check could stop a call with good arguments, so the good path is the GPU test's)"""
    from voxelnet_amd import _lib
    lib = _lib.load()
    table = (_lib.VnEmaChunk * 4)()           # host memory standing in for the device table: never dereferenced
    tab = ctypes.addressof(table)
    assert lib.vn_ema_update(None, 4, 0.1, None) == EINVAL
    for n in (0, -1):
        assert lib.vn_ema_update(tab, n, 0.1, None) == EINVAL
    for w in BAD_WEIGHTS:
        assert lib.vn_ema_update(tab, 4, w, None) == EINVAL, w
        assert lib.vn_ema_update(None, 0, w, None) == EINVAL, w


def test_clip_sgd_ema_argument_checks():
    from voxelnet_amd import _lib
    lib = _lib.load()
    need = lib.vn_clip_sgd_workspace_bytes(1663)
    table = (_lib.VnParamChunkEma * 4)()
    ws = (ctypes.c_char * 64)()
    tab, wsp = ctypes.addressof(table), ctypes.addressof(ws)

    def call(chunks=tab, n_chunks=1663, max_norm=5.0, lr=0.01, w=0.1, ws_ptr=wsp, ws_bytes=need - 1):
        return lib.vn_clip_sgd_ema(chunks, n_chunks, max_norm, lr, 0, w, ws_ptr, ws_bytes, None, None)

    # all arguments good except a workspace one byte short: the last check before the launches
    assert call() == EWORKSPACE and call(ws_bytes=0) == EWORKSPACE
    assert call(w=0.0) == EWORKSPACE and call(w=1.0) == EWORKSPACE
    assert call(max_norm=float("inf")) == EWORKSPACE
    assert call(chunks=None) == EINVAL and call(ws_ptr=None) == EINVAL
    for n in (0, -1):
        assert call(n_chunks=n) == EINVAL
    for mn in (0.0, -5.0, NAN):
        assert call(max_norm=mn) == EINVAL
    for w in BAD_WEIGHTS:
        assert call(w=w) == EINVAL, w
        assert call(w=w, ws_bytes=need) == EINVAL, w          # (good workspace: still refused, nothing launched)


def test_clip_adamw_ema_argument_checks():
    """everything vn_clip_adamw refuses (tests/test_adamw_host.py's list), and the weight"""
    from voxelnet_amd import _lib
    lib = _lib.load()
    need = lib.vn_clip_adamw_workspace_bytes(1663)
    assert need >= 4 * 1663
    table = (_lib.VnAdamChunkEma * 4)()
    ws = (ctypes.c_char * 64)()
    tab, wsp = ctypes.addressof(table), ctypes.addressof(ws)

    def call(chunks=tab, n_chunks=1663, hyper=None, max_norm=5.0, w=0.1, ws_ptr=wsp, ws_bytes=need - 1, null_hyper=False):
        h = None if null_hyper else ctypes.byref(hyper if hyper is not None else _hyper(_lib))
        return lib.vn_clip_adamw_ema(chunks, n_chunks, h, max_norm, 0, w, ws_ptr, ws_bytes, None, None)

    assert call() == EWORKSPACE and call(ws_bytes=0) == EWORKSPACE
    assert call(w=0.0) == EWORKSPACE and call(w=1.0) == EWORKSPACE
    assert call(hyper=_hyper(_lib, 8)) == EWORKSPACE and call(hyper=_hyper(_lib, 3, step=7)) == EWORKSPACE
    assert call(hyper=_hyper(_lib, beta1=0.0, beta2=0.0, eps=0.0, lr=0.0, weight_decay=0.0)) == EWORKSPACE     # the closed ends
    assert call(max_norm=float("inf")) == EWORKSPACE
    for w in BAD_WEIGHTS:
        assert call(w=w) == EINVAL, w
        assert call(w=w, ws_bytes=need) == EINVAL, w
    assert call(chunks=None) == EINVAL
    assert call(null_hyper=True) == EINVAL
    assert call(ws_ptr=None) == EINVAL
    for n in (0, -1):
        assert call(n_chunks=n) == EINVAL
    for mn in (0.0, -5.0, NAN):
        assert call(max_norm=mn) == EINVAL
    for ns in (0, -1, 9, 1 << 20):
        assert call(hyper=_hyper(_lib, ns)) == EINVAL
    bad = [("beta1", 1.0), ("beta1", -0.1), ("beta1", NAN), ("beta2", 1.0), ("beta2", 1.5), ("beta2", -1e-3), ("beta2", NAN),
           ("eps", -1e-8), ("eps", NAN), ("lr", -1e-3), ("lr", NAN), ("weight_decay", -0.01), ("weight_decay", NAN),
           ("step", 0), ("step", -4)]
    for name, value in bad:
        assert call(hyper=_hyper(_lib, 1, **{name: value})) == EINVAL, (name, value)
        assert call(hyper=_hyper(_lib, 5, **{name: value})) == EINVAL, (name, value, "slot 4 of 5")
    h = _hyper(_lib, 2)
    h.slot[2].beta1 = 2.0                      # a bad value beyond n_slots is not looked at
    assert call(hyper=h) == EWORKSPACE


def _net():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7), torch.nn.Linear(7, 3))


def test_the_schedule_against_its_closed_forms():
    from voxelnet_amd.ema import ModelEMA, ema_decay
    assert ema_decay(0, 0.999, 10) == 0.1 == R.decay_at(0)
    # (1 + n) / (10 + n) < 0.999  <=>  n < 8990: the warm-up rules up to n = 8989, the constant from 8990 on
    for n in list(range(0, 200)) + [1000, 5000, 8988, 8989]:
        want = (1.0 + n) / (10.0 + n)
        assert want < 0.999
        assert ema_decay(n, 0.999, 10) == want == R.decay_at(n), n
    assert ema_decay(8989, 0.999, 10) == 8990.0 / 8999.0
    for n in (8990, 8991, 10 ** 6):
        assert ema_decay(n, 0.999, 10) == 0.999 == R.decay_at(n), n
    for warm in (None, 0):
        for n in (0, 1, 7, 8990, 10 ** 6):
            assert ema_decay(n, 0.999, warm) == 0.999 == R.decay_at(n, 0.999, warm)
    # the object walks the same values: n = num_updates before the update
    ema = ModelEMA(_net(), decay=0.999, warmup=10)
    for n in (0, 1, 2, 8989, 8990, 8991):
        ema.num_updates = n
        assert ema.current_decay() == R.decay_at(n) and ema._weight() == R.weight_at(n)
    assert ModelEMA(_net(), decay=0.9, warmup=None).current_decay() == 0.9
    for kw in (dict(decay=1.5), dict(decay=-0.1), dict(warmup=-1)):
        with pytest.raises(ValueError):
            ModelEMA(_net(), **kw)


def test_model_ema_on_cpu_tensors():
    from voxelnet_amd import _lib
    from voxelnet_amd.ema import ModelEMA
    net = _net()
    ema = ModelEMA(net, decay=0.99, warmup=4)
    sd = net.state_dict()
    floats = [k for k, v in sd.items() if v.is_floating_point()]
    assert "1.num_batches_tracked" in sd and "1.num_batches_tracked" not in floats and "1.running_var" in floats
    # one flat buffer, every tensor on a 16-byte boundary, initialised as a copy
    base = ema._flat.data_ptr()
    for k, v in zip(ema._keys, ema._views):
        assert v.data_ptr() % 16 == 0 and base <= v.data_ptr() < base + 4 * ema._flat.numel()
        assert torch.equal(v, sd[k]) and v.data_ptr() != sd[k].data_ptr()
    assert ema._keys == floats
    # model_state_dict: the model's keys in the model's order, the live integer buffers, and it loads
    msd = ema.model_state_dict()
    assert list(msd) == list(sd)
    assert msd["1.num_batches_tracked"].data_ptr() == sd["1.num_batches_tracked"].data_ptr()
    _net().load_state_dict(msd)
    # no CPU path
    with pytest.raises(_lib.VoxelnetHipError):
        ema.update()
    assert ema.num_updates == 0
    # the state-dict round trip: values by key, the three scalars, and copies (not views of the shadow)
    with torch.no_grad():
        for v in ema._views:
            v.add_(1.5)
    ema.num_updates = 7
    state = ema.state_dict()
    assert sorted(state) == ["decay", "num_updates", "shadow", "warmup"] and list(state["shadow"]) == floats
    assert all(t.data_ptr() != v.data_ptr() for t, v in zip(state["shadow"].values(), ema._views))
    other = ModelEMA(_net(), decay=0.5, warmup=None)
    ptrs = [v.data_ptr() for v in other._views]
    other.load_state_dict(state)
    assert (other.decay, other.warmup, other.num_updates) == (0.99, 4, 7)
    assert all(torch.equal(a, b) for a, b in zip(other._views, ema._views))
    assert ptrs == [v.data_ptr() for v in other._views]             # loaded in place
    bad = dict(state, shadow={k: v for k, v in state["shadow"].items() if k != "0.bias"})
    with pytest.raises(KeyError):
        other.load_state_dict(bad)
    # applied(): values exchanged and restored, storage kept, also when the body raises (pure copies: works anywhere)
    live0 = {k: v.clone() for k, v in sd.items()}
    lptrs = [sd[k].data_ptr() for k in floats]
    shadow0 = [v.clone() for v in ema._views]
    with ema.applied():
        assert all(torch.equal(net.state_dict()[k], s) for k, s in zip(floats, shadow0))
        assert all(torch.equal(v, live0[k]) for k, v in zip(floats, ema._views))
    with pytest.raises(RuntimeError, match="boom"):
        with ema.applied():
            raise RuntimeError("boom")
    assert all(torch.equal(net.state_dict()[k], live0[k]) for k in sd)
    assert all(torch.equal(v, s) for v, s in zip(ema._views, shadow0))
    assert lptrs == [net.state_dict()[k].data_ptr() for k in floats]


def test_tied_tensors_are_refused():
    """one tensor under two state-dict keys would get two shadows of which only one is ever averaged"""
    from voxelnet_amd.ema import ModelEMA
    net = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Linear(4, 4))
    net[1].weight = net[0].weight
    with pytest.raises(ValueError, match="one tensor"):
        ModelEMA(net)


def test_attachment_is_not_part_of_the_optimizer_state():
    import copy
    from voxelnet_amd import _lib
    from voxelnet_amd.ema import ModelEMA
    from voxelnet_amd.optim import ClipAdamW, ClipSGD
    net = _net()
    opt = ClipSGD(net.parameters(), lr=0.01, max_norm=5.0)
    opt._table = object()
    ema = ModelEMA(net, opt)
    assert opt._ema is ema and opt._table is None and ema._optimizer is opt          # attach_ema forgets the table
    assert opt._step_table(list(net.parameters()), [torch.zeros_like(p) for p in net.parameters()]) is False
    with pytest.raises(_lib.VoxelnetHipError, match="attached"):
        ema.update()
    assert "_ema" not in opt.state_dict() and all("ema" not in k for k in opt.state_dict()["param_groups"][0])
    assert copy.deepcopy(opt)._ema is None
    # moving to another optimizer detaches the first; None detaches
    other = ClipAdamW(net.parameters())
    other.attach_ema(ema)
    assert opt._ema is None and other._ema is ema and ema._optimizer is other
    other.attach_ema(None)
    assert other._ema is None and ema._optimizer is None
