"""Restatement of the rules of vn_clip_adamw / voxelnet_amd.optim.ClipAdamW in NumPy, written from the rules alone (it shares
no code with the package): torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.AdamW's single-tensor
update with decoupled weight decay, amsgrad=False, maximize=False.

    total = sqrt(sum g^2) over ALL tensors that have a gradient;   coef = min(1, max_norm / (total + 1e-6))
    g' = g * coef;   p <- p * (1 - lr * wd);   m <- m + (g' - m) * (1 - beta1);   v <- beta2 * v + (1 - beta2) * g'^2
    p <- p - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)          t = 1, 2, ... per tensor

`dtype` is the type of every array and of every arithmetic step on arrays: float64 is the reference, float32 is the same
restatement at the kernels' precision — the distance between the two runs on the same inputs is what the tests' bars are
made of (bars()).  The hyperparameter scalars (1 - beta, 1 - lr * wd, the bias corrections) are formed in Python floats
and rounded to `dtype` when they meet an array, which is what torch does and what the library is handed."""
import numpy as np


class RefClipAdamW:
    """params: list of arrays (copied).  groups: list of dicts with `idx` (indices into params) and lr / betas / eps /
    weight_decay, read at every step (a test plays the scheduler by changing them)."""

    def __init__(self, params, groups, max_norm, dtype=np.float64):
        self.dtype = dtype
        self.p = [np.array(p, dtype=dtype) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.groups = groups
        self.max_norm = max_norm

    def step(self, grads):
        """grads: list of arrays or None (a None tensor is skipped: no update, no step count, nothing in the norm).
        -> (total norm before clipping, the scaled gradients g')"""
        dt = self.dtype
        gs = [None if g is None else np.array(g, dtype=dt) for g in grads]
        sq = dt(0)
        for g in gs:
            if g is not None:
                sq = dt(sq + np.sum(g * g, dtype=dt))
        total = dt(np.sqrt(sq))
        coef = dt(dt(self.max_norm) / dt(total + dt(1e-6)))
        if coef > 1:
            coef = dt(1)
        scaled = [None if g is None else g * coef for g in gs]
        for grp in self.groups:
            lr, (b1, b2), eps, wd = grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"]
            for i in grp["idx"]:
                g = scaled[i]
                if g is None:
                    continue
                self.t[i] += 1
                t = self.t[i]
                p = self.p[i] * dt(1 - lr * wd)
                m = self.m[i] + (g - self.m[i]) * dt(1 - b1)
                v = dt(b2) * self.v[i] + dt(1 - b2) * g * g
                step_size = dt(lr / (1 - b1 ** t))
                denom = np.sqrt(v) / dt(np.sqrt(1 - b2 ** t)) + dt(eps)
                self.p[i], self.m[i], self.v[i] = p - step_size * (m / denom), m, v
        return total, scaled

    def snapshot(self):
        return {"p": [a.copy() for a in self.p], "m": [a.copy() for a in self.m], "v": [a.copy() for a in self.v]}


def run(params, groups_fn, grads_per_step, max_norm, dtype):
    """-> [(norm, scaled, snapshot)] per step.  groups_fn(step index) -> the groups in force at that step."""
    ref = RefClipAdamW(params, groups_fn(0), max_norm, dtype)
    out = []
    for s, grads in enumerate(grads_per_step):
        ref.groups = groups_fn(s)
        norm, scaled = ref.step(grads)
        out.append((norm, scaled, ref.snapshot()))
    return out


FLOOR = 1e-12


def bars(run64, run32):
    """per step, per quantity ("p", "m", "v"): 4 x the largest absolute difference between the float32 and the float64 run
    of the restatement over all tensors at that step (never below FLOOR, for a step at which float32 is exact).  The
    factor 4 covers another summation order for the norm and fused multiply-adds."""
    out = []
    for (_, _, s64), (_, _, s32) in zip(run64, run32):
        out.append({q: max(FLOOR, 4.0 * max(float(np.max(np.abs(a.astype(np.float64) - b))) if b.size else 0.0
                                            for a, b in zip(s32[q], s64[q]))) for q in ("p", "m", "v")})
    return out
