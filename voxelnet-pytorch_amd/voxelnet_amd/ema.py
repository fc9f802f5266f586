"""Exponential moving average of the model's weights (timm ModelEmaV2, mmdet's EMA hook, YOLO's ModelEMA,
torch.optim.swa_utils):

    shadow = lerp(shadow, x, w),   w = 1 - d_n,   d_n = min(decay, (1 + n) / (warmup + n)),  n = num_updates

once per optimizer step for every floating-point tensor of `model.state_dict()` — the parameters AND the BatchNorm running
statistics (timm's rule; the statistics are averaged, not recomputed under the averaged weights).  The arithmetic runs in
the HIP library (csrc/optim.hip), with torch.lerp's rounding:

  * attached to a ClipSGD / ClipAdamW, the parameters that take part in a step are averaged INSIDE the update's second
    launch (vn_clip_sgd_ema / vn_clip_adamw_ema: the parameter value is in a register there) and everything else — the
    running statistics, parameters without a gradient this step — by ONE vn_ema_update launch on the same stream right after;
  * on its own (`ema.update()` after a torch optimizer's step), all of it is that one vn_ema_update launch.

Either way every shadowed tensor is lerped exactly once per step with the same w, and the two ways give the same bits.
There is no CPU path: the library must be present and the tensors on a HIP device (fp32, contiguous)."""
import contextlib
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

CHUNK = 4096    # VN_OPT_CHUNK (include/voxelnet_hip.h)
_EMA_ROW = np.dtype([("src", "<u8"), ("ema", "<u8"), ("n", "<i4"), ("reserved", "<i4")])
assert _EMA_ROW.itemsize == ctypes.sizeof(_lib.VnEmaChunk)


def ema_decay(num_updates, decay, warmup):
    """d_n, in Python floats: min(decay, (1 + n) / (warmup + n)); warmup None or 0: decay"""
    if not warmup:
        return float(decay)
    return min(float(decay), (1.0 + num_updates) / (float(warmup) + num_updates))


class ModelEMA:
    """`ModelEMA(model, optimizer=None, decay=0.999, warmup=10)`.

    The shadow is ONE flat fp32 buffer on the model's device with every tensor on a 16-byte boundary (the kernels' vector
    path), initialised as a copy of the model; integer buffers (num_batches_tracked) are not shadowed, the live ones are
    used.  Build it after the model is where it will train: the shadow does not follow a later `model.to()`.  Floating-point
    tensors must be fp32.

    optimizer: a ClipSGD / ClipAdamW to attach to (`optimizer.attach_ema(ema)` does the same later); its step() then
    updates the average and `update()` must not be called as well.  Without one, call `update()` after every optimizer step.
    The attachment is not part of either state dict: after `optimizer.load_state_dict` into a NEW optimizer, or
    `ema.load_state_dict` into a new ModelEMA, attach again.

    `with ema.applied():` runs its body with the averaged weights in the model (values exchanged by copies, the
    parameters' storage and every device table stay); `model.evaluate(..., ema=ema)` does that around its loop.
    `model_state_dict()` is the averaged model as a state dict."""

    def __init__(self, model, optimizer=None, decay=0.999, warmup=10):
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"Invalid decay: {decay}")
        if warmup is not None and warmup < 0:
            raise ValueError(f"Invalid warmup: {warmup}")
        self.model = model
        self.decay, self.warmup, self.num_updates = float(decay), warmup, 0
        sd = model.state_dict(keep_vars=True)
        self._keys = [k for k, t in sd.items() if t.is_floating_point()]
        if not self._keys:
            raise ValueError("ModelEMA: the model has no floating-point tensors")
        self._live = [sd[k] for k in self._keys]
        if any(t.dtype != torch.float32 for t in self._live):
            raise _lib.VoxelnetHipError("ModelEMA: fp32 parameters and buffers only")
        seen = {}
        for k, t in zip(self._keys, self._live):
            if id(t) in seen:
                # (two shadows of one tensor: the optimizer's launch would average one of them and the follow-up launch,
                # which leaves out what the optimizer took, neither)
                raise ValueError(f"ModelEMA: {seen[id(t)]} and {k} are one tensor; tied tensors are not supported")
            seen[id(t)] = k
        offs, total = [], 0
        for t in self._live:
            offs.append(total)
            total += (t.numel() + 3) // 4 * 4
        self._flat = torch.zeros(total, dtype=torch.float32, device=self._live[0].device)
        self._views = [self._flat[o:o + t.numel()].view_as(t) for o, t in zip(offs, self._live)]
        with torch.no_grad():
            for v, t in zip(self._views, self._live):
                v.copy_(t)
        self._by_id = {id(t): v for t, v in zip(self._live, self._views)}
        self._optimizer = None
        self._own = None          # (key, _table(...)) of update(): the table over every shadowed tensor, keyed on the live pointers
        if optimizer is not None:
            optimizer.attach_ema(self)

    # ---- the schedule ---------------------------------------------------------------------------------------------------
    def current_decay(self):
        """d_n of the NEXT update"""
        return ema_decay(self.num_updates, self.decay, self.warmup)

    def _weight(self):
        return 1.0 - self.current_decay()

    # ---- tables ---------------------------------------------------------------------------------------------------------
    def shadow(self, tensor):
        """the shadow view of a live parameter / buffer of the model, or None when it is not shadowed"""
        return self._by_id.get(id(tensor))

    def _shadow_ptr(self, tensor):
        v = self._by_id.get(id(tensor))
        return 0 if v is None else v.data_ptr()

    def _rest_table(self, fused, dev):
        """the vn_ema_update table of every shadowed tensor that is NOT among `fused` (the parameters an attached
        optimizer's own launch averages) -> (device table, chunks, elements), or None when nothing is left"""
        skip = {id(p) for p in fused}
        pairs = [(t, v) for t, v in zip(self._live, self._views) if id(t) not in skip]
        return self._table(pairs, dev)

    def _table(self, pairs, dev):
        if self._flat.device != dev:
            raise _lib.VoxelnetHipError("ModelEMA: the shadow and the model's tensors must live on one HIP device (no CPU path)")
        for t, _ in pairs:
            if not (t.is_cuda and t.device == dev):
                raise _lib.VoxelnetHipError("ModelEMA: the shadow and the model's tensors must live on one HIP device (no CPU path)")
            if not t.is_contiguous():
                raise _lib.VoxelnetHipError("ModelEMA: contiguous tensors only")
        rows = [(t.data_ptr() + 4 * off, v.data_ptr() + 4 * off, min(CHUNK, t.numel() - off), 0)
                for t, v in pairs for off in range(0, t.numel(), CHUNK)]
        if not rows:
            return None
        table = torch.from_numpy(np.array(rows, dtype=_EMA_ROW).view(np.uint8).copy()).to(dev)
        return table, len(rows), sum(t.numel() for t, _ in pairs)

    def _launch(self, table, w):
        """one vn_ema_update over `table` on the current stream"""
        if table is None:
            return
        with _lib.on_device(self._flat.device):
            from . import engine as E
            with E.section("ema_update", 12.0 * table[2]):          # source read, shadow read + written
                _lib.call("vn_ema_update", table[0].data_ptr(), table[1], w, _lib.raw_stream())

    def _after_step(self, rest, w):
        """an attached optimizer's step: its own launch has averaged the parameters with weight w; the rest follows"""
        self._launch(rest, w)
        self.num_updates += 1

    @torch.no_grad()
    def update(self):
        """one update of every shadowed tensor from the model as it is now (after a torch optimizer's step)"""
        if self._optimizer is not None:
            raise _lib.VoxelnetHipError("ModelEMA.update: attached to an optimizer, whose step() updates the average")
        dev = self._flat.device
        if dev.type != "cuda" or not all(t.is_cuda for t in self._live):
            raise _lib.VoxelnetHipError("ModelEMA: the shadow and the model's tensors must live on one HIP device (no CPU path)")
        key = [t.data_ptr() for t in self._live]
        if self._own is None or self._own[0] != key:
            self._own = (key, self._table(list(zip(self._live, self._views)), dev))
        self._launch(self._own[1], self._weight())
        self.num_updates += 1

    # ---- the averaged model ---------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _exchange(self):
        """live <-> shadow, values only: every tensor keeps its storage (the optimizers' chunk tables and the executor's
        pointer arrays hold raw pointers); the copies are in place, so anything keyed on a tensor's version sees them"""
        held = self._flat.clone()
        off_views = [held[v.storage_offset():v.storage_offset() + v.numel()].view_as(v) for v in self._views]
        live = [t.detach() for t in self._live]
        torch._foreach_copy_(self._views, live)
        torch._foreach_copy_(live, off_views)

    @contextlib.contextmanager
    def applied(self):
        """the model holds the averaged weights (and averaged running statistics) inside, the shadow holds the live ones;
        restored on exit, also when the body raises.  Do not step the optimizer inside."""
        self._exchange()
        try:
            yield self
        finally:
            self._exchange()

    def model_state_dict(self):
        """the averaged model: the shadow under the model's state-dict keys (views of the flat buffer, not copies) plus the
        live integer buffers; `RPN3D(...).load_state_dict(ema.model_state_dict())` gives the model evaluate(ema=) scores"""
        byk = dict(zip(self._keys, self._views))
        out = OrderedDict()
        for k, t in self.model.state_dict().items():
            out[k] = byk[k] if k in byk else t
        return out

    # ---- state ----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """decay, warmup, num_updates and a copy of the shadow by state-dict key (the attachment is not part of it)"""
        return {"decay": self.decay, "warmup": self.warmup, "num_updates": self.num_updates,
                "shadow": OrderedDict((k, v.detach().clone()) for k, v in zip(self._keys, self._views))}

    @torch.no_grad()
    def load_state_dict(self, state):
        shadow = state["shadow"]
        if set(shadow) != set(self._keys):
            missing, extra = sorted(set(self._keys) - set(shadow)), sorted(set(shadow) - set(self._keys))
            raise KeyError(f"ModelEMA.load_state_dict: missing {missing}, unexpected {extra}")
        for k, v in zip(self._keys, self._views):
            if tuple(shadow[k].shape) != tuple(v.shape):
                raise ValueError(f"ModelEMA.load_state_dict: {k} has shape {tuple(shadow[k].shape)}, expected {tuple(v.shape)}")
        for k, v in zip(self._keys, self._views):
            v.copy_(shadow[k])          # in place: the shadow's storage (and every table that names it) stays
        self.decay, self.warmup, self.num_updates = float(state["decay"]), state["warmup"], int(state["num_updates"])
