"""Float64 NumPy restatement of the weight average: the decay schedule and the lerp.  Shares no code with
the package.

    d_n = min(decay, (1 + n) / (warmup + n)),  n = number of updates so far;  warmup None / 0: d_n = decay
    w_n = 1 - d_n
    ema <- ema + w * (x - ema)

The library takes the weight as a C float.  `weight32(w)` is that float, widened again: the reference averages with the
weight the library was handed, so that the error bound below counts the arithmetic's roundings only.

Bound of one step on float32 inputs, per element: |got - ref| <= 2^-22 * max(|ema|, |x|).  One rounding of x - ema
(<= 2^-24 of a magnitude <= 2 max) and one of the fmaf (<= 2^-24 of a magnitude <= max, the result lying between ema and
x; counted as 2 max): 4 * 2^-24.  Over k steps the errors add (each later step scales an earlier error by 1 - w <= 1)."""
import numpy as np

STEP_EPS = 2.0 ** -22


def decay_at(n, decay=0.999, warmup=10):
    if warmup is None or warmup == 0:
        return float(decay)
    return min(float(decay), (1.0 + n) / (float(warmup) + n))


def weight_at(n, decay=0.999, warmup=10):
    return 1.0 - decay_at(n, decay, warmup)


def weight32(w):
    return float(np.float32(w))


def lerp(ema, x, w):
    """one update in float64 from arrays of any float type, weight as the library receives it"""
    e, x = np.asarray(ema, dtype=np.float64), np.asarray(x, dtype=np.float64)
    return e + weight32(w) * (x - e)


def step_bound(ema, x):
    """the bound of one step, elementwise, from the step's float32 inputs"""
    return STEP_EPS * np.maximum(np.abs(np.asarray(ema, dtype=np.float64)), np.abs(np.asarray(x, dtype=np.float64)))


def run(start, sequence, decay=0.999, warmup=10, n0=0):
    """the shadow after averaging `sequence` (a list of arrays: the recorded values of one tensor after each step) into
    `start`, update counts n0, n0 + 1, ... -> (float64 shadow, elementwise bound: the sum of the steps' bounds, each taken
    from the float64 shadow before the step and the recorded value)"""
    e = np.asarray(start, dtype=np.float64).copy()
    bound = np.zeros_like(e)
    for k, x in enumerate(sequence):
        bound += step_bound(e, x)
        e = lerp(e, x, weight_at(n0 + k, decay, warmup))
    return e, bound
