"""Weight average on the device (csrc/optim.hip: vn_ema_update, vn_clip_sgd_ema, vn_clip_adamw_ema; voxelnet_amd.ema.ModelEMA)
against tests/ema_ref.py, the float64 NumPy restatement of the schedule and the lerp.

Tolerance: derived, not measured.  One update on float32 inputs: |got - ref| <= 2^-22 * max(|ema|, |x|) per element — one
rounding of x - ema and one of the fmaf, each at most 2^-24 of a magnitude of at most 2 max (ema_ref.step_bound); the
reference averages with the weight as the library receives it (a C float).  k updates: the sum of the k steps' bounds, which
is at most k times the largest.  Every comparison prints bar, observed error and their ratio before it asserts.

Tensors: tests/test_gpu_adamw.py's SHAPES — chunk tails 4097 and 8191, one-element tensors — as separate tensors or as views
of one flat buffer that start off 16-byte boundaries (the kernels' element-by-element path)."""
import functools

import numpy as np
import pytest
import torch

import ema_ref as R
from test_gpu_adamw import BASE, DECAY, DEV, MAX_NORM, REST, SHAPES, place, set_grads

pytestmark = pytest.mark.gpu
BUFFERS = [(4097,), (7,), (1,)]          # floating-point buffers of the test module: averaged by the follow-up launch


@functools.lru_cache(maxsize=None)
def inputs(scale, steps, seed=11):
    """(parameters, [gradients per step], [buffer values per step]) as CPU tensors, computed once and never written"""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    gs = [[torch.randn(s, generator=g) * scale for s in SHAPES] for _ in range(steps)]
    bs = [[torch.randn(s, generator=g) for s in BUFFERS] for _ in range(steps + 1)]
    return ps, gs, bs


class Bag(torch.nn.Module):
    """SHAPES as parameters p0..p8 (placed separately or in one flat buffer), BUFFERS as float buffers, one integer buffer"""

    def __init__(self, ps, bufs, flat):
        super().__init__()
        for i, t in enumerate(place(ps, flat)):
            self.register_parameter(f"p{i}", torch.nn.Parameter(t))
        for i, t in enumerate(bufs):
            self.register_buffer(f"b{i}", t.to(DEV).clone())
        self.register_buffer("count", torch.zeros((), dtype=torch.int64, device=DEV))

    def plist(self):
        return [getattr(self, f"p{i}") for i in range(len(SHAPES))]

    def blist(self):
        return [getattr(self, f"b{i}") for i in range(len(BUFFERS))]

    def tick(self, values):
        """what a train-mode forward does to the buffers: new running statistics, the counter + 1"""
        with torch.no_grad():
            for b, v in zip(self.blist(), values):
                b.copy_(v)
            self.count += 1


def make(kind, ps, bufs, flat, scale_grads=False, ema=True, **ema_kw):
    from voxelnet_amd.ema import ModelEMA
    from voxelnet_amd.optim import ClipAdamW, ClipSGD
    bag = Bag(ps, bufs, flat)
    params = bag.plist()
    if kind == "sgd":
        opt = ClipSGD(params, lr=0.01, max_norm=MAX_NORM, scale_grads=scale_grads)
    else:
        opt = ClipAdamW([dict(params=[params[i] for i in DECAY], lr=2e-3, weight_decay=0.01),
                         dict(params=[params[i] for i in REST], lr=1e-3, weight_decay=0.0)],
                        max_norm=MAX_NORM, scale_grads=scale_grads, **BASE)
    avg = ModelEMA(bag, opt if ema else None, **ema_kw)
    return bag, params, opt, avg


def shadow_of(avg):
    return [v.clone() for v in avg._views]


def moments(opt, params):
    return [opt.state[p][k] for p in params for k in ("exp_avg", "exp_avg_sq") if k in opt.state.get(p, {})]


def all_equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def check_bound(tag, got, ref, bound):
    """got: tensors; ref, bound: float64 arrays, elementwise bound; prints before it asserts"""
    worst, worst_err, worst_bar, n = 0.0, 0.0, 0.0, 0
    for a, r, b in zip(got, ref, bound):
        err = np.abs(a.detach().double().cpu().numpy() - r)
        assert np.all(np.isfinite(err))
        ratio = np.where(err > 0, err / np.where(b > 0, b, 1e-300), 0.0)
        k = int(np.argmax(ratio))
        if ratio.flat[k] >= worst:
            worst, worst_err, worst_bar = float(ratio.flat[k]), float(err.flat[k]), float(b.flat[k])
        n += err.size
    print(f"{tag}: bar {worst_bar:.3e} observed {worst_err:.3e} ratio {worst:.3f} (worst of {n} elements, elementwise bar)")
    assert worst <= 1.0, (tag, worst)


# ---- 1. vn_ema_update alone ----------------------------------------------------------------------------------------------
SIZES = [(1,), (3,), (4095,), (4096,), (4097,)]
GUARD = 4          # sentinel elements behind every shadow tensor
SENTINEL = -777.25


@functools.lru_cache(maxsize=None)
def alone_inputs():
    g = torch.Generator().manual_seed(23)
    shapes = SHAPES + SIZES
    return [torch.randn(s, generator=g) for s in shapes], [torch.randn(s, generator=g) * 3.0 for s in shapes]


def alone_place(flat):
    """-> source tensors, shadow tensors, the guards behind the shadows.  flat: both sides are views of one buffer each and
    start off 16-byte boundaries (sources back to back, shadows GUARD + 1 apart); separate: own allocations"""
    xs, es = alone_inputs()
    src = place(xs, flat)
    if flat:
        buf = torch.full((sum(e.numel() + GUARD + 1 for e in es),), SENTINEL, device=DEV)
    shadow, guards, off = [], [], 1
    for e in es:
        n = e.numel()
        if not flat:
            buf, off = torch.full((n + GUARD,), SENTINEL, device=DEV), 0
        shadow.append(buf[off:off + n].view_as(e).copy_(e))
        guards.append(buf[off + n:off + n + GUARD])
        off += n + GUARD + 1
    return src, shadow, guards


def ema_update(src, shadow, w):
    """vn_ema_update through the binding, table built here"""
    from voxelnet_amd import _lib
    from voxelnet_amd.ema import _EMA_ROW, CHUNK
    rows = [(x.data_ptr() + 4 * o, e.data_ptr() + 4 * o, min(CHUNK, x.numel() - o), 0)
            for x, e in zip(src, shadow) for o in range(0, x.numel(), CHUNK)]
    table = torch.from_numpy(np.array(rows, dtype=_EMA_ROW).view(np.uint8).copy()).to(DEV)
    _lib.call("vn_ema_update", table.data_ptr(), len(rows), w, _lib.raw_stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("w", [0.001, 0.1, 0.5, 0.9])
def test_ema_update_alone_matches_float64(w, flat):
    xs, es = alone_inputs()
    src, shadow, guards = alone_place(flat)
    assert any(t.data_ptr() % 16 for t in src + shadow) == flat
    ema_update(src, shadow, w)
    ref = [R.lerp(e.numpy(), x.numpy(), w) for e, x in zip(es, xs)]
    bound = [R.step_bound(e.numpy(), x.numpy()) for e, x in zip(es, xs)]
    check_bound(f"alone[w={w} flat={flat}]", shadow, ref, bound)
    assert all(torch.equal(s.cpu(), x) for s, x in zip(src, xs))                      # the sources are read only
    assert all(bool((g == SENTINEL).all()) for g in guards)
    moved = sum(int((s.cpu() != e).sum()) for s, e in zip(shadow, es))
    assert moved > 0.99 * sum(e.numel() for e in es)


@pytest.mark.parametrize("flat", [False, True])
def test_ema_update_alone_closed_ends_and_null(flat):
    from voxelnet_amd import _lib
    from voxelnet_amd.ema import _EMA_ROW
    xs, es = alone_inputs()
    src, shadow, guards = alone_place(flat)
    ema_update(src, shadow, 0.0)                                                      # w = 0: the shadow stays, bit for bit
    assert all(torch.equal(s.cpu(), e) for s, e in zip(shadow, es))
    ema_update(src, shadow, 1.0)                                                      # w = 1: a copy, bit for bit
    assert all(torch.equal(s.cpu(), x) for s, x in zip(shadow, xs))
    assert all(bool((g == SENTINEL).all()) for g in guards)
    # a row without a shadow or without a source is left out
    a, b = torch.ones(5, device=DEV), torch.zeros(5, device=DEV)
    rows = [(a.data_ptr(), 0, 5, 0), (0, b.data_ptr(), 5, 0), (a.data_ptr(), b.data_ptr(), 2, 0)]
    table = torch.from_numpy(np.array(rows, dtype=_EMA_ROW).view(np.uint8).copy()).to(DEV)
    _lib.call("vn_ema_update", table.data_ptr(), 3, 0.5, _lib.raw_stream())
    assert b.tolist() == [0.5, 0.5, 0.0, 0.0, 0.0] and a.tolist() == [1.0] * 5


# ---- 2. fused = unfused, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("scale", [1.0, 1e-4])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("scale_grads", [False, True])
def test_fused_average_is_the_plain_step_plus_ema_update(kind, scale, flat, scale_grads):
    """six steps with the average attached (vn_clip_*_ema + the follow-up launch) against a twin whose optimizer knows of no
    average and whose ModelEMA runs update() (one vn_ema_update over everything) after each step"""
    from voxelnet_amd import _lib
    ps, gs, bs = inputs(scale, 6)
    names = []
    real_call = _lib.call

    def counting_call(name, *args):
        names.append(name)
        return real_call(name, *args)

    a_bag, a_params, a_opt, a_avg = make(kind, ps, bs[0], flat, scale_grads, ema=True)
    b_bag, b_params, b_opt, b_avg = make(kind, ps, bs[0], flat, scale_grads, ema=False)
    assert a_opt._ema is a_avg and b_opt._ema is None
    for s in range(6):
        for bag, params, opt, avg in ((a_bag, a_params, a_opt, a_avg), (b_bag, b_params, b_opt, b_avg)):
            set_grads(params, gs[s], flat)
            bag.tick(bs[s + 1])
        names.clear()
        _lib.call = counting_call
        try:
            na = a_opt.step()
            fused_names = list(names)
            names.clear()
            nb = b_opt.step()
            b_avg.update()
            plain_names = list(names)
        finally:
            _lib.call = real_call
        assert fused_names == [f"vn_clip_{kind}_ema", "vn_ema_update"] and plain_names == [f"vn_clip_{kind}", "vn_ema_update"]
        tag = (kind, scale, flat, scale_grads, s)
        assert torch.equal(na, nb), tag
        assert bool(na > MAX_NORM) == (scale == 1.0)                                  # clip active / idle
        assert all_equal([p.detach() for p in a_params], [p.detach() for p in b_params]), tag
        assert all_equal(moments(a_opt, a_params), moments(b_opt, b_params)), tag
        assert all_equal([p.grad for p in a_params], [p.grad for p in b_params]), tag
        assert all_equal(a_avg._views, b_avg._views), tag
        assert a_avg.num_updates == b_avg.num_updates == s + 1
    # the average did move, buffers included, and sits between where it started and where the model is
    start = [t.to(DEV) for t in ps] + [t.to(DEV) for t in bs[0]]
    assert all(not torch.equal(v, t) for v, t in zip(a_avg._views, start) if v.numel() > 1)
    assert int(a_bag.count) == 6


# ---- 3. against float64 over a run; 4. against torch on the device -------------------------------------------------------
def test_six_steps_match_float64_on_the_recorded_sequence():
    ps, gs, bs = inputs(1.0, 6)
    bag, params, opt, avg = make("adamw", ps, bs[0], True, warmup=10)
    start = [v.cpu().numpy() for v in avg._views]
    seq = [[] for _ in avg._views]
    for s in range(6):
        set_grads(params, gs[s], True)
        bag.tick(bs[s + 1])
        opt.step()
        for k, t in enumerate(avg._live):
            seq[k].append(t.detach().cpu().numpy().copy())
    assert [R.decay_at(n) for n in range(3)] == [0.1, 2.0 / 11.0, 0.25] and avg.num_updates == 6
    runs = [R.run(s0, sq, 0.999, 10) for s0, sq in zip(start, seq)]
    # the bar: the six steps' bounds added up — at most 6 x the largest single-step bound
    for (_, b), s0, sq in zip(runs, start, seq):
        big = np.maximum(np.abs(s0.astype(np.float64)), np.max(np.abs(np.asarray(sq, dtype=np.float64)), axis=0))
        assert np.all(b <= 6 * R.STEP_EPS * big * (1 + 1e-12))
    check_bound("six_steps vs float64", avg._views, [r for r, _ in runs], [b for _, b in runs])


def test_one_step_matches_torch_lerp_on_the_device():
    """constant decay 0.999; per step torch.lerp(shadow before, parameter after, w) against the shadow after: both are
    within one step bound of float64, so within two of each other.  Prints the fraction of bit-equal elements."""
    ps, gs, bs = inputs(1.0, 6)
    bag, params, opt, avg = make("adamw", ps, bs[0], False, decay=0.999, warmup=None)
    w = 1.0 - 0.999
    equal = total = 0
    for s in range(3):
        set_grads(params, gs[s], False)
        bag.tick(bs[s + 1])
        before = shadow_of(avg)
        assert avg._weight() == w
        opt.step()
        want = [torch.lerp(e, t.detach(), w) for e, t in zip(before, avg._live)]
        bound = [2 * R.step_bound(e.cpu().numpy(), t.detach().cpu().numpy()) for e, t in zip(before, avg._live)]
        check_bound(f"vs torch.lerp step {s + 1}", avg._views, [t.double().cpu().numpy() for t in want], bound)
        equal += sum(int((a == b).sum()) for a, b in zip(avg._views, want))
        total += sum(a.numel() for a in want)
    print(f"vs torch.lerp: {equal} of {total} elements bit-equal ({equal / total:.6f})")


# ---- 5. a parameter without a gradient ------------------------------------------------------------------------------------
def test_a_parameter_without_a_gradient_is_averaged_by_the_follow_up_launch():
    from voxelnet_amd.ema import _EMA_ROW
    from voxelnet_amd.optim import _ADAM_EMA_ROW
    ps, gs, bs = inputs(1.0, 6)
    a_bag, a_params, a_opt, a_avg = make("adamw", ps, bs[0], False, ema=True)
    b_bag, b_params, b_opt, b_avg = make("adamw", ps, bs[0], False, ema=False)
    ptrs = [v.data_ptr() for v in a_avg._views]
    OUT = 6                                                                # (8191,): two chunks
    lo = a_avg.shadow(a_params[OUT]).data_ptr()
    hi = lo + 4 * a_params[OUT].numel()

    def tables():
        fused = a_opt._table.cpu().numpy().view(_ADAM_EMA_ROW)
        rest = a_opt._ema_rest[0].cpu().numpy().view(_EMA_ROW)
        return (int(((fused["ema"] >= lo) & (fused["ema"] < hi)).sum()), int(((rest["ema"] >= lo) & (rest["ema"] < hi)).sum()),
                len(fused), len(rest))

    for s in range(3):
        for bag, params in ((a_bag, a_params), (b_bag, b_params)):
            bag.tick(bs[s + 1])
            for i, (p, g) in enumerate(zip(params, gs[s])):
                p.grad = None if (s == 1 and i == OUT) else g.to(DEV)
        before = a_avg.shadow(a_params[OUT]).clone()
        kept = a_params[OUT].detach().clone()
        w = a_avg._weight()
        a_opt.step()
        b_opt.step()
        b_avg.update()
        n_fused, n_rest, rows_fused, rows_rest = tables()
        if s == 1:
            assert (n_fused, n_rest) == (0, 2) and torch.equal(a_params[OUT].detach(), kept)
            # its shadow moved all the same, by this step's w
            now = a_avg.shadow(a_params[OUT])
            assert not torch.equal(now, before)
            check_bound("sat out: shadow vs float64", [now], [R.lerp(before.cpu().numpy(), kept.cpu().numpy(), w)],
                        [R.step_bound(before.cpu().numpy(), kept.cpu().numpy())])
        else:
            assert (n_fused, n_rest) == (2, 0)
        assert rows_fused + rows_rest == sum((t.numel() + 4095) // 4096 for t in a_avg._live)
        assert all_equal(a_avg._views, b_avg._views) and all_equal([p.detach() for p in a_params], [p.detach() for p in b_params])
        assert ptrs == [v.data_ptr() for v in a_avg._views]                 # the rebuilds keep the shadow's storage
    assert a_avg.num_updates == 3


# ---- 6. applied() -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_applied_exchanges_values_and_nothing_else(kind):
    ps, gs, bs = inputs(1.0, 6)
    a_bag, a_params, a_opt, a_avg = make(kind, ps, bs[0], True)
    b_bag, b_params, b_opt, b_avg = make(kind, ps, bs[0], True)          # the twin never swaps
    uploads = []
    real_upload = a_opt._upload

    def counting_upload(rows, *args):
        key_before = a_opt._key
        real_upload(rows, *args)
        uploads.append(a_opt._key != key_before)

    a_opt._upload = counting_upload
    for s in range(3):
        for bag, params, opt in ((a_bag, a_params, a_opt), (b_bag, b_params, b_opt)):
            set_grads(params, gs[s], True)
            bag.tick(bs[s + 1])
            opt.step()
    table, rebuilt = a_opt._table, sum(uploads)
    assert rebuilt == 1
    live0 = [t.detach().clone() for t in a_avg._live]
    shadow0 = shadow_of(a_avg)
    lptrs, sptrs = [t.data_ptr() for t in a_avg._live], [v.data_ptr() for v in a_avg._views]
    assert not all_equal(live0, shadow0)
    with a_avg.applied() as inside:
        assert inside is a_avg
        assert all_equal([t.detach() for t in a_avg._live], shadow0) and all_equal(a_avg._views, live0)
        assert int(a_bag.count) == 3                                       # the integer buffer is the live one
        sd = a_bag.state_dict()
        assert all(torch.equal(sd[k], v) for k, v in zip(a_avg._keys, shadow0))
    with pytest.raises(RuntimeError, match="boom"):
        with a_avg.applied():
            raise RuntimeError("boom")
    assert all_equal([t.detach() for t in a_avg._live], live0) and all_equal(a_avg._views, shadow0)
    assert lptrs == [t.data_ptr() for t in a_avg._live] and sptrs == [v.data_ptr() for v in a_avg._views]
    for s in range(3, 6):
        for bag, params, opt in ((a_bag, a_params, a_opt), (b_bag, b_params, b_opt)):
            set_grads(params, gs[s], True)
            bag.tick(bs[s + 1])
        na, nb = a_opt.step(), b_opt.step()
        assert torch.equal(na, nb)
        assert all_equal([p.detach() for p in a_params], [p.detach() for p in b_params])
        assert all_equal(moments(a_opt, a_params), moments(b_opt, b_params))
        assert all_equal(a_avg._views, b_avg._views)
    assert a_opt._table is table and sum(uploads) == rebuilt               # no table was rebuilt because of a swap


# ---- 8. two runs, and resuming -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_two_runs_are_bit_equal_and_a_loaded_average_continues(kind):
    from voxelnet_amd.ema import ModelEMA
    ps, gs, bs = inputs(1.0, 6)
    runs = []
    for resume in (False, False, True):
        bag, params, opt, avg = make(kind, ps, bs[0], True, scale_grads=True)
        norms = []
        for s in range(6):
            if resume and s == 3:
                state = avg.state_dict()
                with torch.no_grad():
                    for v in avg._views:
                        v.fill_(float("nan"))                               # the old average is gone
                avg = ModelEMA(bag, decay=0.5, warmup=None)
                avg.load_state_dict(state)
                opt.attach_ema(avg)
                assert avg.num_updates == 3 and avg.decay == 0.999 and avg.warmup == 10
            set_grads(params, gs[s], True)
            bag.tick(bs[s + 1])
            norms.append(opt.step().clone())
        runs.append((norms, [p.detach() for p in params], moments(opt, params), shadow_of(avg), avg.num_updates))
    for other in runs[1:]:
        assert all_equal(runs[0][0], other[0]) and all_equal(runs[0][1], other[1]) and all_equal(runs[0][2], other[2])
        assert all_equal(runs[0][3], other[3]) and other[4] == 6
    assert all(bool(torch.isfinite(v).all()) for v in runs[2][3])


def test_cpu_shadow_or_cpu_model_raises_on_the_device_path():
    from voxelnet_amd import _lib
    from voxelnet_amd.ema import ModelEMA
    from voxelnet_amd.optim import ClipSGD
    net = torch.nn.Linear(3, 2)
    avg = ModelEMA(net)                                                     # built while the model was on the CPU
    net.to(DEV)
    with pytest.raises(_lib.VoxelnetHipError):
        avg.update()
    opt = ClipSGD(net.parameters(), 0.01, 5.0)
    opt.attach_ema(avg)
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in net.parameters()]
    with pytest.raises(_lib.VoxelnetHipError):
        opt.step()
    assert all_equal(before, [p.detach() for p in net.parameters()]) and avg.num_updates == 0


# ---- 7. the detector --------------------------------------------------------------------------------------------------------
def _detector_setup():
    from voxelnet_amd import synth
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.voxelize import voxelize_device
    grid = grid_config("Car")
    frames = synth.workload_frames(1, batch=1, frame0=0)
    feats, coords = [], []
    for b, f in enumerate(frames):
        fb, cb, _ = voxelize_device(torch.from_numpy(f).to(DEV), grid, b, coord_cols=4)
        feats.append(fb)
        coords.append(cb)
    labels = [synth.synth_labels("Car", 3, 40)]
    return (["000000"], labels, feats, None, coords, None, None)


def _detector(seed=5):
    from voxelnet_amd import model as M
    torch.manual_seed(seed)
    model = M.RPN3D("Car").to(DEV).train(True)
    h, w = model.rpn_output_shape
    g = torch.Generator().manual_seed(3)
    pos = (torch.rand((1, h, w, 2), generator=g) < 0.02).float().to(DEV)
    neg = (1 - pos) * (torch.rand((1, h, w, 2), generator=g) < 0.9).float().to(DEV)
    tgt = (torch.randn((1, h, w, 14), generator=g) * 0.3).to(DEV)
    return model, (pos, neg, tgt)


def test_detector_train_steps_with_an_average_and_its_evaluation():
    """Whole detector (the setup of test_gpu_adamw's train-step test: Car grid, batch 1, bf16, given targets), five
    train_steps with ClipAdamW: with a ModelEMA attached the step's outputs, the parameters and the moments are those of
    the run without one, bit for bit; the shadows of the BatchNorm running statistics follow the float64 average of the
    recorded statistics; evaluate(ema=) scores what a second module loaded from model_state_dict() scores."""
    from voxelnet_amd import model as M
    from voxelnet_amd.ema import ModelEMA
    from voxelnet_amd.optim import ClipAdamW, decay_param_groups
    from voxelnet_amd.predict import EVAL_DECODE
    before = M.get_precision()
    M.set_precision("bf16")
    try:
        x = _detector_setup()
        results = {}
        for arm in ("ema", "plain"):
            model, targets = _detector()
            params = list(model.parameters())
            opt = ClipAdamW(decay_param_groups(model, 0.01), lr=2e-4, max_norm=MAX_NORM, **BASE)
            avg = ModelEMA(model, opt) if arm == "ema" else None
            outs, stats = [], []
            if avg is not None:
                stat_idx = [i for i, k in enumerate(avg._keys) if "running_" in k]
                assert len(stat_idx) == 50 and len(avg._keys) == 104 + 50
                start = [avg._views[i].cpu().numpy() for i in stat_idx]
            for _ in range(5):
                for p in params:
                    p.grad = None
                out = model.train_step(x, DEV, opt, targets=targets)
                outs.append([t.clone() for t in out] + [opt._norm.clone()])
                if avg is not None:
                    stats.append([avg._live[i].detach().cpu().numpy().copy() for i in stat_idx])
            results[arm] = (outs, [p.detach().clone() for p in params], moments(opt, params))
            if arm == "ema":
                kept = (model, avg, stat_idx, start, stats)
        for a, b in zip(results["ema"][0], results["plain"][0]):
            assert all_equal(a, b)
        assert all_equal(results["ema"][1], results["plain"][1]) and all_equal(results["ema"][2], results["plain"][2])
        model, avg, stat_idx, start, stats = kept
        assert avg.num_updates == 5
        runs = [R.run(s0, [st[k] for st in stats], 0.999, 10) for k, s0 in enumerate(start)]
        check_bound("detector: running-statistics shadows vs float64", [avg._views[i] for i in stat_idx],
                    [r for r, _ in runs], [b for _, b in runs])
        assert not any(torch.equal(avg._views[i], avg._live[i]) for i in stat_idx)
        # evaluation under the average
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        shadow = shadow_of(avg)
        ev = model.evaluate([x], DEV, decode=EVAL_DECODE, ema=avg)
        got = ev.compute()
        assert model.training and all(torch.equal(v, state[k]) for k, v in model.state_dict().items())
        assert all_equal(avg._views, shadow)
        second = M.RPN3D("Car")
        second.load_state_dict(avg.model_state_dict())
        second = second.to(DEV).eval()
        ev2 = second.evaluate([x], DEV, decode=EVAL_DECODE)
        want = ev2.compute()
        # ... and the other way round: after the exchange back the module scores its own weights again — what a third module
        # loaded from the state saved before the evaluation scores — and that is not what the average scores
        live = model.evaluate([x], DEV, decode=EVAL_DECODE)
        got_live = live.compute()
        third = M.RPN3D("Car")
        third.load_state_dict(state)
        third = third.to(DEV).eval()
        ev3 = third.evaluate([x], DEV, decode=EVAL_DECODE)
        want_live = ev3.compute()
        assert len(ev._pending) == len(ev2._pending) == len(live._pending) == len(ev3._pending) == 1
        (st_a, sc_a, _, _), (st_b, sc_b, _, _), (st_l, sc_l, _, _) = ev._pending[0], ev2._pending[0], live._pending[0]
        st_3, sc_3 = ev3._pending[0][:2]
        assert torch.equal(st_l, st_3) and torch.equal(sc_l, sc_3) and repr(got_live) == repr(want_live)
        print(f"detector: {got['n_det']} detections under the average; {int((sc_a != sc_l).sum())} of {sc_a.numel()} score "
              "slots differ from the live weights' evaluation")
        assert got["n_det"] > 0
        assert got_live["n_det"] > 0 and not torch.equal(sc_a, sc_l)
        assert torch.equal(st_a, st_b) and torch.equal(sc_a, sc_b)
        assert repr(got) == repr(want)                                       # (NaN-safe: AP of an empty class is NaN)
        with pytest.raises(ValueError):
            second.evaluate([x], DEV, ema=avg)                               # another module's average
    finally:
        M.set_precision(before)


def test_detector_train_step_with_clip_sgd_and_an_average():
    """a ClipSGD with an average attached: train_step runs the update after the library call (vnStep carries the plain table
    only), parameters bit-equal to train_step(x, DEV, None) + step() of a plain ClipSGD"""
    from voxelnet_amd import _lib
    from voxelnet_amd import model as M
    from voxelnet_amd.ema import ModelEMA
    from voxelnet_amd.optim import ClipSGD
    before = M.get_precision()
    M.set_precision("bf16")
    names = []
    real_call = _lib.call

    def counting_call(name, *args):
        names.append(name)
        return real_call(name, *args)

    try:
        x = _detector_setup()
        results = {}
        for arm in ("ema", "plain"):
            model, targets = _detector()
            params = list(model.parameters())
            opt = ClipSGD(params, 0.01, MAX_NORM)
            avg = ModelEMA(model, opt) if arm == "ema" else None
            snaps = []
            for _ in range(2):
                for p in params:
                    p.grad = None
                if arm == "ema":
                    assert model._step_fused_ok("bf16", opt)
                    _lib.call = counting_call
                    try:
                        model.train_step(x, DEV, opt, targets=targets)
                    finally:
                        _lib.call = real_call
                else:
                    model.train_step(x, DEV, None, targets=targets)
                    opt.step()
                snaps.append([p.detach().clone() for p in params] + [opt._norm.clone()])
            results[arm] = snaps
            if avg is not None:
                assert avg.num_updates == 2
                # (a bias in front of a BatchNorm may see a gradient of exactly zero and stay where it was)
                assert sum(not torch.equal(v, t.detach()) for v, t in zip(avg._views, avg._live)) >= 100
        assert names.count("vn_net_step") == 2 and names.count("vn_clip_sgd_ema") == 2 and names.count("vn_ema_update") == 2
        assert "vn_clip_sgd" not in names
        for a, b in zip(results["ema"], results["plain"]):
            assert all_equal(a, b)
    finally:
        M.set_precision(before)
