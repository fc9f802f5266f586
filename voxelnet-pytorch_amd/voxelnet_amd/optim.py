"""Optimizer tail of the reference's train step (voxelnet/train.py:153-154):

    clip_grad_norm_(model.parameters(), 5)        # train.py:153
    optimizer.step()                              # train.py:154, optimizer = SGD(model.parameters(), lr=0.01)

as two HIP launches (csrc/optim.hip, `vn_clip_sgd`) over a device chunk table of the (parameter, gradient) pairs,
whatever their placement (the module's flat gradient buffer, the DDP buckets' views, or 104 separate tensors).
No CPU / torch fallback: the HIP library must be present.

`ClipAdamW` is the same tail with torch.optim.AdamW in SGD's place (what SECOND, PointPillars and their successors train
with): csrc/adamw.hip, `vn_clip_adamw`, again two launches, over (parameter, gradient, exp_avg, exp_avg_sq) chunks."""
import ctypes

import numpy as np
import torch

from . import _lib

CHUNK = 4096    # VN_OPT_CHUNK (include/voxelnet_hip.h)


class ClipSGD(torch.optim.Optimizer):
    """`ClipSGD(params, lr, max_norm).step()` == `clip_grad_norm_(params, max_norm); SGD(params, lr).step()`.
    step() returns the total gradient norm before clipping (a device scalar, clip_grad_norm_'s return value).

    A torch.optim.Optimizer: `param_groups` / `state_dict()` / `load_state_dict()` / `zero_grad()` are the base class's, so
    the reference's `MultiStepLR(optimizer, ...)` (train.py:131) attaches and its lr changes are honoured: the learning
    rate is read from `param_groups[0]["lr"]` at every step.  The norm is taken over ALL parameters together (as
    train.py:153 does), so every group must carry the same lr / max_norm."""

    def __init__(self, params, lr, max_norm, scale_grads=False):
        defaults = dict(lr=float(lr), max_norm=float(max_norm), scale_grads=bool(scale_grads))
        super().__init__(params, defaults)
        if not any(len(g["params"]) for g in self.param_groups):
            raise ValueError("ClipSGD got an empty parameter list")
        self._key = None
        self._table = self._ws = self._norm = None
        self._n_chunks = 0
        self._plist = self._last_grads = self._last_pptrs = self._fused_key = None

    # (kept for callers of the round-1 class)
    @property
    def params(self):
        return [p for g in self.param_groups for p in g["params"]]

    @property
    def lr(self):
        return float(self.param_groups[0]["lr"])

    @property
    def max_norm(self):
        return float(self.param_groups[0]["max_norm"])

    @property
    def scale_grads(self):
        return bool(self.param_groups[0]["scale_grads"])

    def __setstate__(self, state):        # (the base class pickles defaults / state / param_groups only)
        super().__setstate__(state)
        self._key = None                  # device chunk table / workspace: rebuilt on the first step
        self._table = self._ws = self._norm = None
        self._n_chunks = 0
        self._plist = self._last_grads = self._last_pptrs = self._fused_key = None

    def zero_grad(self, set_to_none=True):
        """torch.optim.Optimizer.zero_grad without its per-parameter foreach bookkeeping (104 small tensors)"""
        if not set_to_none:
            return super().zero_grad(set_to_none=False)
        for p in self.params:
            p.grad = None

    def add_param_group(self, group):
        super().add_param_group(group)
        self._plist = self._last_grads = self._last_pptrs = self._fused_key = None

    def _build(self, pairs, dev):
        rows = []
        for p, g in pairs:
            n, pp, gp = p.numel(), p.data_ptr(), g.data_ptr()
            for off in range(0, n, CHUNK):
                rows.append((pp + 4 * off, gp + 4 * off, min(CHUNK, n - off), 0))
        tab = np.array(rows, dtype=np.dtype([("param", "<u8"), ("grad", "<u8"), ("n", "<i4"), ("reserved", "<i4")]))
        assert tab.dtype.itemsize == ctypes.sizeof(_lib.VnParamChunk)
        self._table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
        self._n_chunks = len(rows)
        nbytes = _lib.load().vn_clip_sgd_workspace_bytes(self._n_chunks)
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._norm = torch.zeros(1, dtype=torch.float32, device=dev)

    def _step_table(self, params, grads):
        """RPN3D.train_step (vn_net_step): make sure the device chunk table covers exactly the pairs (params[i], grads[i]) —
        the gradients are not attached to the parameters yet, the update runs inside the library call — and that this
        optimizer's parameters are those.  -> True: _table / _ws / _norm are valid for the call; False: use step()."""
        for g in self.param_groups[1:]:
            if g["lr"] != self.param_groups[0]["lr"] or g["max_norm"] != self.param_groups[0]["max_norm"]:
                return False
        plist = self.__dict__.get("_plist")
        if plist is None:
            plist = self._plist = self.params
        pptrs = [p.data_ptr() for p in params]
        hit = self.__dict__.get("_fused_key")
        if hit is not None and hit[0] is params and hit[1] is grads and hit[2] == pptrs and self._table is not None:
            return True
        if len(plist) != len(params) or {id(p) for p in plist} != {id(p) for p in params}:
            return False
        dev = params[0].device
        for p, g in zip(params, grads):
            if not (p.is_cuda and g.is_cuda and p.device == dev and g.device == dev and p.dtype == torch.float32
                    and g.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous() and p.numel() == g.numel()):
                return False
        gmap = {id(p): g for p, g in zip(params, grads)}
        pairs = [(p, gmap[id(p)]) for p in plist]
        key = tuple((p.data_ptr(), g.data_ptr(), p.numel()) for p, g in pairs)
        if key != self._key:
            self._build(pairs, dev)
            self._key = key
        self._n_elems = sum(p.numel() for p in plist)
        self._last_grads = [gmap[id(p)] for p in plist]      # (step() right after the call would see the same tensors)
        self._last_pptrs = [p.data_ptr() for p in plist]
        self._fused_key = (params, grads, pptrs)
        return True

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise _lib.VoxelnetHipError("ClipSGD.step: closures are not supported")
        for g in self.param_groups[1:]:
            if g["lr"] != self.param_groups[0]["lr"] or g["max_norm"] != self.param_groups[0]["max_norm"]:
                raise _lib.VoxelnetHipError("ClipSGD: one lr / max_norm for all parameter groups (the clip norm is global)")
        plist = self.__dict__.get("_plist")
        if plist is None:
            plist = self._plist = self.params
        last = self.__dict__.get("_last_grads")
        if (last is not None and self._table is not None and all(p.grad is g for p, g in zip(plist, last))
                and self._last_pptrs == [p.data_ptr() for p in plist]):
            # the same gradient tensors as in the previous step (the model's flat buffer / bucket views) and the same
            # parameter storage (a `p.data = ...` / `set_()` swap keeps the Parameter object but not its memory): the chunk
            # table of raw pointers is still valid, nothing to rebuild or re-check
            with _lib.on_device(self._table.device):
                stream = _lib.raw_stream()
                from . import engine as E
                with E.section("clip_sgd", 16.0 * self._n_elems):
                    _lib.call("vn_clip_sgd", self._table.data_ptr(), self._n_chunks, self.max_norm, self.lr,
                              int(self.scale_grads), self._ws.data_ptr(), self._ws.numel(), self._norm.data_ptr(), stream)
            return self._norm[0]
        pairs = [(p, p.grad) for p in plist if p.grad is not None]
        if not pairs:
            return None
        dev = pairs[0][0].device
        for p, g in pairs:
            if not (p.is_cuda and g.is_cuda and p.device == dev and g.device == dev):
                raise _lib.VoxelnetHipError("ClipSGD: parameters and gradients must live on one HIP device (no CPU path)")
            if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous() or not g.is_contiguous():
                raise _lib.VoxelnetHipError("ClipSGD: fp32 contiguous parameters and gradients only")
        key = tuple((p.data_ptr(), g.data_ptr(), p.numel()) for p, g in pairs)
        if key != self._key:
            self._build(pairs, dev)        # pointers are stable from step to step (flat gradient buffer): built once
            self._key = key
        self._n_elems = sum(p.numel() for p, _ in pairs)
        self._last_grads = [p.grad for p in plist] if len(pairs) == len(plist) else None
        self._last_pptrs = [p.data_ptr() for p in plist]
        with _lib.on_device(dev):
            stream = _lib.raw_stream()
            from . import engine as E
            with E.section("clip_sgd", 16.0 * sum(p.numel() for p, _ in pairs)):      # grad read twice, param read + written
                _lib.call("vn_clip_sgd", self._table.data_ptr(), self._n_chunks, self.max_norm, self.lr, int(self.scale_grads),
                          self._ws.data_ptr(), self._ws.numel(), self._norm.data_ptr(), stream)
        return self._norm[0]


def decay_param_groups(model, weight_decay):
    """The "no decay on BatchNorm and biases" idiom as two parameter groups for ClipAdamW / torch.optim.AdamW: tensors with
    dim() > 1 (convolution and linear weights) take `weight_decay`, everything else (biases, BatchNorm affine parameters) 0."""
    params = [p for p in model.parameters() if p.requires_grad]
    return [{"params": [p for p in params if p.dim() > 1], "weight_decay": float(weight_decay)},
            {"params": [p for p in params if p.dim() <= 1], "weight_decay": 0.0}]


class ClipAdamW(torch.optim.Optimizer):
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
        if not any(len(g["params"]) for g in self.param_groups):
            raise ValueError("ClipAdamW got an empty parameter list")
        self._forget()

    def _forget(self):
        """drop everything derived from param_groups / state: the device chunk table is rebuilt on the next step"""
        self._key = None
        self._table = self._ws = self._norm = None
        self._n_chunks = self._n_elems = 0
        self._plist = self._pgroup = self._last_grads = self._last_pptrs = None
        self._slots = self._steps = None
        self._hyper = _lib.VnAdamHyper()

    @property
    def params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def __setstate__(self, state):        # unpickling, copy.deepcopy and the tail of load_state_dict
        super().__setstate__(state)
        for g in self.param_groups:       # (a torch.optim.AdamW state dict has no max_norm / scale_grads)
            for k, v in self.defaults.items():
                g.setdefault(k, v)
        self._forget()

    def zero_grad(self, set_to_none=True):
        """torch.optim.Optimizer.zero_grad without its per-parameter foreach bookkeeping (104 small tensors)"""
        if not set_to_none:
            return super().zero_grad(set_to_none=False)
        for p in self.params:
            p.grad = None

    def add_param_group(self, group):
        super().add_param_group(group)
        self._forget()

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

    def _build(self, rows, dev):
        tab = np.array(rows, dtype=np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"),
                                             ("n", "<i4"), ("slot", "<i4")]))
        assert tab.dtype.itemsize == ctypes.sizeof(_lib.VnAdamChunk)
        self._table = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
        self._n_chunks = len(rows)
        nbytes = _lib.load().vn_clip_adamw_workspace_bytes(self._n_chunks)
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._norm = torch.zeros(1, dtype=torch.float32, device=dev)

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
            with E.section("clip_adamw", 32.0 * self._n_elems):      # grad read twice; p, m, v read + written
                _lib.call("vn_clip_adamw", self._table.data_ptr(), self._n_chunks, ctypes.byref(h), float(g0["max_norm"]),
                          int(bool(g0["scale_grads"])), self._ws.data_ptr(), self._ws.numel(), self._norm.data_ptr(), stream)
        for s in self._slots:
            s[1] += 1
        self._steps += 1          # every taking-part parameter's state["step"] is a view of this CPU buffer

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise _lib.VoxelnetHipError("ClipAdamW.step: closures are not supported")
        g0 = self.param_groups[0]
        for g in self.param_groups[1:]:
            if g["max_norm"] != g0["max_norm"] or bool(g["scale_grads"]) != bool(g0["scale_grads"]):
                raise _lib.VoxelnetHipError("ClipAdamW: one max_norm / scale_grads for all parameter groups (the clip norm is global)")
        plist = self._plist
        if plist is None:
            plist = self._plist = self.params
            self._pgroup = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        last = self._last_grads
        if (last is not None and self._table is not None and all(p.grad is g for p, g in zip(plist, last))
                and self._last_pptrs == [p.data_ptr() for p in plist]):
            # the same gradient tensors as in the previous step (the model's flat buffer / bucket views), the same parameter
            # storage and — no load_state_dict / add_param_group since, which call _forget — the same state tensors: the
            # chunk table of raw pointers is still valid and every step count went up by one together
            self._launch()
            return self._norm[0]
        pairs = [(i, p) for i, p in enumerate(plist) if p.grad is not None]
        if not pairs:
            return None
        dev = pairs[0][1].device
        for _, p in pairs:
            g = p.grad
            if not (p.is_cuda and g.is_cuda and p.device == dev and g.device == dev):
                raise _lib.VoxelnetHipError("ClipAdamW: parameters and gradients must live on one HIP device (no CPU path)")
            if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous() or not g.is_contiguous():
                raise _lib.VoxelnetHipError("ClipAdamW: fp32 contiguous parameters and gradients only")
        fresh = [p for _, p in pairs if len(self.state.get(p, ())) == 0]
        if fresh:
            self._new_state(fresh)
        slots, rows, steps = {}, [], []
        for i, p in pairs:
            st = self.state[p]
            m, v = st["exp_avg"], st["exp_avg_sq"]
            for t_ in (m, v):
                if not (t_.is_cuda and t_.device == dev and t_.dtype == torch.float32 and t_.is_contiguous()
                        and t_.numel() == p.numel()):
                    raise _lib.VoxelnetHipError("ClipAdamW: exp_avg / exp_avg_sq must be fp32 contiguous tensors of the "
                                                "parameter's size on its device")
            t = int(float(st["step"]))
            steps.append(float(t))
            slot = slots.setdefault((self._pgroup[i], t), len(slots))
            n, pp, gp, mp, vp = p.numel(), p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr()
            for off in range(0, n, CHUNK):
                rows.append((pp + 4 * off, gp + 4 * off, mp + 4 * off, vp + 4 * off, min(CHUNK, n - off), slot))
        if len(slots) > _lib.VN_OPT_MAX_SLOTS:
            raise _lib.VoxelnetHipError(
                f"ClipAdamW: the parameters of this step fall into {len(slots)} distinct (parameter group, step count) "
                f"combinations, and one call carries at most {_lib.VN_OPT_MAX_SLOTS} hyperparameter sets: use fewer groups, or "
                "keep the step counts together (parameters skipped for want of a gradient fall behind the others)")
        key = tuple(rows)
        if key != self._key:
            self._build(rows, dev)        # pointers are stable from step to step (flat gradient buffer): built once
            self._key = key
        # the step counters of the parameters taking part move into one CPU buffer (one add per step instead of one per
        # parameter); a counter that arrived through load_state_dict is copied, not aliased
        self._steps = torch.tensor(steps, dtype=torch.float32)
        for j, (_, p) in enumerate(pairs):
            self.state[p]["step"] = self._steps[j]
        self._slots = [[gi, t] for (gi, t) in slots]
        self._n_elems = sum(p.numel() for _, p in pairs)
        self._last_grads = [p.grad for p in plist] if len(pairs) == len(plist) else None
        self._last_pptrs = [p.data_ptr() for p in plist]
        self._launch()
        return self._norm[0]
