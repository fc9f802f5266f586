"""Optimizer tail of the reference's train step (voxelnet/train.py:153-154):

    clip_grad_norm_(model.parameters(), 5)        # train.py:153
    optimizer.step()                              # train.py:154, optimizer = SGD(model.parameters(), lr=0.01)

as two HIP launches (csrc/optim.hip, `vn_clip_sgd`) over a device chunk table of the (parameter, gradient) pairs,
whatever their placement (the module's flat gradient buffer, the DDP buckets' views, or 104 separate tensors).
No CPU / torch fallback: the HIP library must be present.

`ClipAdamW` is the same tail with torch.optim.AdamW in SGD's place (what SECOND, PointPillars and their successors train
with): the same file's other update rule, `vn_clip_adamw`, again two launches, over (parameter, gradient, exp_avg,
exp_avg_sq) chunks.  What the two classes share — the chunk table's life and the checks — is `_ClipOptimizer`.

Either class takes a weight average along (`attach_ema`, voxelnet_amd/ema.py): the chunks then carry the shadow's pointer
and the second launch averages the parameter it has just computed (`vn_clip_sgd_ema`, `vn_clip_adamw_ema`)."""
import ctypes

import numpy as np
import torch

from . import _lib

CHUNK = 4096    # VN_OPT_CHUNK (include/voxelnet_hip.h)
_SGD_ROW = np.dtype([("param", "<u8"), ("grad", "<u8"), ("n", "<i4"), ("reserved", "<i4")])
_ADAM_ROW = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("n", "<i4"), ("slot", "<i4")])
assert _SGD_ROW.itemsize == ctypes.sizeof(_lib.VnParamChunk) and _ADAM_ROW.itemsize == ctypes.sizeof(_lib.VnAdamChunk)
_SGD_EMA_ROW = np.dtype([("param", "<u8"), ("grad", "<u8"), ("ema", "<u8"), ("n", "<i4"), ("reserved", "<i4")])
_ADAM_EMA_ROW = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("ema", "<u8"), ("n", "<i4"),
                          ("slot", "<i4")])
assert _SGD_EMA_ROW.itemsize == ctypes.sizeof(_lib.VnParamChunkEma)
assert _ADAM_EMA_ROW.itemsize == ctypes.sizeof(_lib.VnAdamChunkEma)


class _ClipOptimizer(torch.optim.Optimizer):
    """The part of the tail that does not depend on the update rule: a device chunk table of raw pointers, built when the
    tensors of a step are not those of the step before and dropped (_forget) whenever param_groups or state change hands.
    A subclass supplies _check_groups(), _prepare(taking, dev) -> the table's rows, and _launch()."""

    _ema = None       # an attached ema.ModelEMA (class-level default: the attachment does not travel with a pickle / deepcopy)

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        if not any(len(g["params"]) for g in self.param_groups):
            raise ValueError(f"{type(self).__name__} got an empty parameter list")
        self._forget()

    def _forget(self):
        """drop everything derived from param_groups / state: the device chunk table is rebuilt on the next step"""
        self._key = None
        self._table = self._ws = self._norm = None
        self._n_chunks = self._n_elems = 0
        self._plist = self._last_grads = self._last_pptrs = None
        self._ema_rest = None

    def attach_ema(self, ema):
        """Average the weights into `ema` (an ema.ModelEMA, or None to detach) as part of every step(): the parameters that
        take part in the step inside the update's second launch, every other shadowed tensor (BatchNorm running statistics,
        parameters without a gradient this step) by one vn_ema_update launch on the same stream right after — so each
        shadowed tensor is averaged once per step, with one weight.  A step() that finds no gradient at all does nothing,
        the average included.  The attachment is not part of state_dict(): attach again after loading into a new optimizer."""
        if self._ema is not None:
            self._ema._optimizer = None
        self._ema = ema
        if ema is not None:
            if ema._optimizer is not None and ema._optimizer is not self:
                ema._optimizer.attach_ema(None)
            ema._optimizer = self
        self._forget()

    def _ema_rows(self, taking, dev):
        """the attached average's side of _prepare: the follow-up launch's table for what `taking` leaves out"""
        self._ema_rest = self._ema._rest_table([p for _, p in taking if self._ema.shadow(p) is not None], dev)

    # (kept for callers of the round-1 class)
    @property
    def params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def __setstate__(self, state):        # unpickling, copy.deepcopy and the tail of load_state_dict
        super().__setstate__(state)       # (the base class pickles defaults / state / param_groups only)
        self._forget()

    def add_param_group(self, group):
        super().add_param_group(group)
        self._forget()

    def zero_grad(self, set_to_none=True):
        """torch.optim.Optimizer.zero_grad without its per-parameter foreach bookkeeping (104 small tensors)"""
        if not set_to_none:
            return super().zero_grad(set_to_none=False)
        for p in self.params:
            p.grad = None

    def _params(self):
        if self._plist is None:
            self._plist = self.params
        return self._plist

    def _check(self, dev, *tensors):
        if not all(t.is_cuda and t.device == dev for t in tensors):
            raise _lib.VoxelnetHipError(f"{type(self).__name__}: parameters and gradients must live on one HIP device (no CPU path)")
        if not all(t.dtype == torch.float32 and t.is_contiguous() for t in tensors):
            raise _lib.VoxelnetHipError(f"{type(self).__name__}: fp32 contiguous parameters and gradients only")

    @staticmethod
    def _cut(ptrs, n, last):
        """the rows of one tensor tuple: its base pointers advanced chunk by chunk (a 0 — no shadow — stays 0), the chunk's
        length, the last column"""
        return [tuple(b and b + 4 * off for b in ptrs) + (min(CHUNK, n - off), last) for off in range(0, n, CHUNK)]

    def _upload(self, rows, dtype, workspace_fn, dev):
        """table, workspace and norm for `rows`; pointers are stable from step to step (flat gradient buffer): built once"""
        key = tuple(rows)
        if key == self._key:
            return
        self._table = torch.from_numpy(np.array(rows, dtype=dtype).view(np.uint8).copy()).to(dev)
        self._n_chunks = len(rows)
        self._ws = torch.empty(getattr(_lib.load(), workspace_fn)(self._n_chunks), dtype=torch.uint8, device=dev)
        self._norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self._key = key

    def _same_tensors(self, plist):
        """the same gradient tensors as in the previous step (the model's flat buffer / bucket views), the same parameter
        storage (a `p.data = ...` / `set_()` swap keeps the Parameter object but not its memory) and — no load_state_dict
        / add_param_group since, which call _forget — the same state tensors: the chunk table of raw pointers is still
        valid, nothing to rebuild or re-check"""
        last = self._last_grads
        return (last is not None and self._table is not None and all(p.grad is g for p, g in zip(plist, last))
                and self._last_pptrs == [p.data_ptr() for p in plist])

    def _remember(self, plist, grads, n_elems):
        """`grads`: every parameter's gradient tensor in plist's order, or None when some parameter has none"""
        self._n_elems = n_elems
        self._last_grads = grads
        self._last_pptrs = [p.data_ptr() for p in plist]

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise _lib.VoxelnetHipError(f"{type(self).__name__}.step: closures are not supported")
        self._check_groups()
        plist = self._params()
        if not self._same_tensors(plist):
            taking = [(i, p) for i, p in enumerate(plist) if p.grad is not None]
            if not taking:
                return None
            dev = taking[0][1].device
            for _, p in taking:
                self._check(dev, p, p.grad)
            self._prepare(taking, dev)
            self._remember(plist, [p.grad for p in plist] if len(taking) == len(plist) else None,
                           sum(p.numel() for _, p in taking))
        self._launch()
        return self._norm[0]


class ClipSGD(_ClipOptimizer):
    """`ClipSGD(params, lr, max_norm).step()` == `clip_grad_norm_(params, max_norm); SGD(params, lr).step()`.
    step() returns the total gradient norm before clipping (a device scalar, clip_grad_norm_'s return value).

    A torch.optim.Optimizer: `param_groups` / `state_dict()` / `load_state_dict()` / `zero_grad()` are the base class's, so
    the reference's `MultiStepLR(optimizer, ...)` (train.py:131) attaches and its lr changes are honoured: the learning
    rate is read from `param_groups[0]["lr"]` at every step.  The norm is taken over ALL parameters together (as
    train.py:153 does), so every group must carry the same lr / max_norm."""

    def __init__(self, params, lr, max_norm, scale_grads=False):
        super().__init__(params, dict(lr=float(lr), max_norm=float(max_norm), scale_grads=bool(scale_grads)))

    def _forget(self):
        super()._forget()
        self._fused_key = None

    @property
    def lr(self):
        return float(self.param_groups[0]["lr"])

    @property
    def max_norm(self):
        return float(self.param_groups[0]["max_norm"])

    @property
    def scale_grads(self):
        return bool(self.param_groups[0]["scale_grads"])

    def _one_lr(self):
        g0 = self.param_groups[0]
        return all(g["lr"] == g0["lr"] and g["max_norm"] == g0["max_norm"] for g in self.param_groups[1:])

    def _check_groups(self):
        if not self._one_lr():
            raise _lib.VoxelnetHipError("ClipSGD: one lr / max_norm for all parameter groups (the clip norm is global)")

    def _prepare(self, taking, dev):
        ema = self._ema
        if ema is None:
            rows = [r for _, p in taking for r in self._cut((p.data_ptr(), p.grad.data_ptr()), p.numel(), 0)]
            self._upload(rows, _SGD_ROW, "vn_clip_sgd_workspace_bytes", dev)
            return
        self._ema_rows(taking, dev)          # (first: it checks that the shadow lives on `dev`)
        rows = [r for _, p in taking for r in self._cut((p.data_ptr(), p.grad.data_ptr(), ema._shadow_ptr(p)), p.numel(), 0)]
        self._upload(rows, _SGD_EMA_ROW, "vn_clip_sgd_workspace_bytes", dev)

    def _step_table(self, params, grads):
        """RPN3D.train_step (vn_net_step): make sure the device chunk table covers exactly the pairs (params[i], grads[i]) —
        the gradients are not attached to the parameters yet, the update runs inside the library call — and that this
        optimizer's parameters are those.  -> True: _table / _ws / _norm are valid for the call; False: use step().
        vnStep carries the plain table only: with a weight average attached the update runs after the call."""
        if not self._one_lr() or self._ema is not None:
            return False
        plist = self._params()
        pptrs = [p.data_ptr() for p in params]
        hit = self._fused_key
        if hit is not None and hit[0] is params and hit[1] is grads and hit[2] == pptrs and self._table is not None:
            return True
        if len(plist) != len(params) or {id(p) for p in plist} != {id(p) for p in params}:
            return False
        dev = params[0].device
        try:
            for p, g in zip(params, grads):
                self._check(dev, p, g)
        except _lib.VoxelnetHipError:
            return False
        if any(p.numel() != g.numel() for p, g in zip(params, grads)):
            return False
        gmap = {id(p): g for p, g in zip(params, grads)}
        glist = [gmap[id(p)] for p in plist]
        rows = [r for p, g in zip(plist, glist) for r in self._cut((p.data_ptr(), g.data_ptr()), p.numel(), 0)]
        self._upload(rows, _SGD_ROW, "vn_clip_sgd_workspace_bytes", dev)
        self._remember(plist, glist, sum(p.numel() for p in plist))      # (step() right after the call would see the same tensors)
        self._fused_key = (params, grads, pptrs)
        return True

    def _launch(self):
        with _lib.on_device(self._table.device):
            stream = _lib.raw_stream()
            from . import engine as E
            ema = self._ema
            if ema is None:
                with E.section("clip_sgd", 16.0 * self._n_elems):      # grad read twice, param read + written
                    _lib.call("vn_clip_sgd", self._table.data_ptr(), self._n_chunks, self.max_norm, self.lr, int(self.scale_grads),
                              self._ws.data_ptr(), self._ws.numel(), self._norm.data_ptr(), stream)
                return
            w = ema._weight()
            with E.section("clip_sgd_ema", 24.0 * self._n_elems):      # + the shadow read + written
                _lib.call("vn_clip_sgd_ema", self._table.data_ptr(), self._n_chunks, self.max_norm, self.lr, int(self.scale_grads),
                          w, self._ws.data_ptr(), self._ws.numel(), self._norm.data_ptr(), stream)
            ema._after_step(self._ema_rest, w)


def decay_param_groups(model, weight_decay):
    """The "no decay on BatchNorm and biases" idiom as two parameter groups for ClipAdamW / torch.optim.AdamW: tensors with
    dim() > 1 (convolution and linear weights) take `weight_decay`, everything else (biases, BatchNorm affine parameters) 0."""
    params = [p for p in model.parameters() if p.requires_grad]
    return [{"params": [p for p in params if p.dim() > 1], "weight_decay": float(weight_decay)},
            {"params": [p for p in params if p.dim() <= 1], "weight_decay": 0.0}]


class ClipAdamW(_ClipOptimizer):
    """`ClipAdamW(params, lr, betas, eps, weight_decay, max_norm).step()` ==
    `clip_grad_norm_(params, max_norm); torch.optim.AdamW(params, lr, betas, eps, weight_decay).step()` (single-tensor
    rules, amsgrad=False, maximize=False, decoupled decay).  step() returns the total gradient norm before clipping (a
    device scalar, clip_grad_norm_'s return value).

    Parameter groups may differ in lr / betas / eps / weight_decay (see decay_param_groups); the norm is taken over ALL
    parameters together, so max_norm and scale_grads are global and groups that disagree on them raise.  The
    hyperparameters are read from `param_groups` at every step and handed to the library by value: MultiStepLR and
    OneCycleLR (which finds `betas` in `defaults` and cycles beta1) attach and are honoured without a rebuild of the
    device chunk table.  Every distinct (group, step count) among the parameters that take part in a step is one of the
    library's VN_OPT_MAX_SLOTS hyperparameter slots.  The library takes the hyperparameters as floats: values with up to
    seven significant digits are honoured exactly, others to half a float ulp (include/voxelnet_hip.h).

    State per parameter under torch.optim.AdamW's own keys — `step` (float32 scalar on the CPU), `exp_avg`, `exp_avg_sq`
    (fp32 on the parameter's device, zero at first use) — so `state_dict()` loads into torch.optim.AdamW and back.  New
    moments are views of one flat buffer with every tensor on a 16-byte boundary (the kernel's vector path); moments that
    arrive through load_state_dict are used where they are.  A parameter whose .grad is None is skipped entirely."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=5.0, scale_grads=False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not 0.0 < max_norm:
            raise ValueError(f"Invalid max_norm value: {max_norm}")
        defaults = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay),
                        max_norm=float(max_norm), scale_grads=bool(scale_grads))
        super().__init__(params, defaults)

    def _forget(self):
        super()._forget()
        self._slots = self._steps = None
        self._hyper = _lib.VnAdamHyper()

    def __setstate__(self, state):
        super().__setstate__(state)
        for g in self.param_groups:       # (a torch.optim.AdamW state dict has no max_norm / scale_grads)
            for k, v in self.defaults.items():
                g.setdefault(k, v)

    def _new_state(self, params):
        """zero moments for `params` as views of ONE flat buffer, each tensor on a 16-byte boundary"""
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4
        flat = torch.zeros(2 * total, dtype=torch.float32, device=params[0].device)
        for p, off in zip(params, offs):
            n = p.numel()
            self.state[p] = {"step": torch.tensor(0.0, dtype=torch.float32),
                             "exp_avg": flat[off:off + n].view_as(p), "exp_avg_sq": flat[total + off:total + off + n].view_as(p)}

    def _check_groups(self):
        g0 = self.param_groups[0]
        for g in self.param_groups[1:]:
            if g["max_norm"] != g0["max_norm"] or bool(g["scale_grads"]) != bool(g0["scale_grads"]):
                raise _lib.VoxelnetHipError("ClipAdamW: one max_norm / scale_grads for all parameter groups (the clip norm is global)")

    def _prepare(self, taking, dev):
        if self._ema is not None:
            self._ema_rows(taking, dev)          # (first: it checks that the shadow lives on `dev`, before any state is made)
        fresh = [p for _, p in taking if len(self.state.get(p, ())) == 0]
        if fresh:
            self._new_state(fresh)
        pgroup = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        slots, rows, steps = {}, [], []
        for i, p in taking:
            st = self.state[p]
            m, v = st["exp_avg"], st["exp_avg_sq"]
            for t_ in (m, v):
                if not (t_.is_cuda and t_.device == dev and t_.dtype == torch.float32 and t_.is_contiguous()
                        and t_.numel() == p.numel()):
                    raise _lib.VoxelnetHipError("ClipAdamW: exp_avg / exp_avg_sq must be fp32 contiguous tensors of the "
                                                "parameter's size on its device")
            t = int(float(st["step"]))
            steps.append(float(t))
            slot = slots.setdefault((pgroup[i], t), len(slots))
            ptrs = (p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr())
            rows += self._cut(ptrs if self._ema is None else ptrs + (self._ema._shadow_ptr(p),), p.numel(), slot)
        if len(slots) > _lib.VN_OPT_MAX_SLOTS:
            raise _lib.VoxelnetHipError(
                f"ClipAdamW: the parameters of this step fall into {len(slots)} distinct (parameter group, step count) "
                f"combinations, and one call carries at most {_lib.VN_OPT_MAX_SLOTS} hyperparameter sets: use fewer groups, or "
                "keep the step counts together (parameters skipped for want of a gradient fall behind the others)")
        self._upload(rows, _ADAM_ROW if self._ema is None else _ADAM_EMA_ROW, "vn_clip_adamw_workspace_bytes", dev)
        # the step counters of the parameters taking part move into one CPU buffer (one add per step instead of one per
        # parameter); a counter that arrived through load_state_dict is copied, not aliased
        self._steps = torch.tensor(steps, dtype=torch.float32)
        for j, (_, p) in enumerate(taking):
            self.state[p]["step"] = self._steps[j]
        self._slots = [[gi, t] for (gi, t) in slots]

    def _launch(self):
        """one vn_clip_adamw call for the slots of the current table, hyperparameters as param_groups hold them NOW; then
        the step counters advance"""
        h, groups = self._hyper, self.param_groups
        h.n_slots = len(self._slots)
        for k, (gi, t) in enumerate(self._slots):
            g, s = groups[gi], h.slot[k]
            if g.get("amsgrad") or g.get("maximize"):
                raise _lib.VoxelnetHipError("ClipAdamW: amsgrad / maximize are not implemented")
            s.lr, s.beta1, s.beta2 = float(g["lr"]), float(g["betas"][0]), float(g["betas"][1])
            s.eps, s.weight_decay, s.step = float(g["eps"]), float(g["weight_decay"]), t + 1
        g0 = groups[0]
        with _lib.on_device(self._table.device):
            stream = _lib.raw_stream()
            from . import engine as E
            ema = self._ema
            if ema is None:
                with E.section("clip_adamw", 32.0 * self._n_elems):      # grad read twice; p, m, v read + written
                    _lib.call("vn_clip_adamw", self._table.data_ptr(), self._n_chunks, ctypes.byref(h), float(g0["max_norm"]),
                              int(bool(g0["scale_grads"])), self._ws.data_ptr(), self._ws.numel(), self._norm.data_ptr(), stream)
            else:
                w = ema._weight()
                with E.section("clip_adamw_ema", 40.0 * self._n_elems):      # + the shadow read + written
                    _lib.call("vn_clip_adamw_ema", self._table.data_ptr(), self._n_chunks, ctypes.byref(h), float(g0["max_norm"]),
                              int(bool(g0["scale_grads"])), w, self._ws.data_ptr(), self._ws.numel(), self._norm.data_ptr(), stream)
                ema._after_step(self._ema_rest, w)
        for s in self._slots:
            s[1] += 1
        self._steps += 1          # every taking-part parameter's state["step"] is a view of this CPU buffer
