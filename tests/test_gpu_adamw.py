"""Fused gradient-clip + AdamW tail (csrc/optim.hip through vn_clip_adamw / voxelnet_amd.optim.ClipAdamW) against
tests/adamw_ref.py, the float64 NumPy restatement of clip_grad_norm_ + torch.optim.AdamW's single-tensor rules.

Tolerance: measured, not chosen.  For p, exp_avg and exp_avg_sq the bar at a step is 4 x the largest absolute difference
between the restatement's float32 run and its float64 run on the same inputs at that step (adamw_ref.bars; floor 1e-12);
relative bars are unusable for exp_avg, which cancels.  The norm: 1e-6 relative, tests/test_gpu_optim.py's bar.
Every comparison prints bar, observed error and their ratio before it asserts.

The library takes the hyperparameters as floats and widens each to the double with the shortest decimal form (0.999f
means 0.999); a double that needs more than a float's digits loses up to half a float ulp there — for beta1 that is up
to 3e-8 * |g' - m| per step on exp_avg, which is the size of these bars.  The scheduler test therefore uses a OneCycleLR
whose four beta1 values (0.95, 0.9, 0.85, 0.875) are short decimals; its lr values are arbitrary doubles, whose float
rounding (6e-8 relative on a 1e-3 step) is far below the bar on p."""
import copy
import functools
import pickle

import numpy as np
import pytest
import torch

import adamw_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_NORM = 5.0

# tests/test_gpu_optim.py's list: chunk tails, one-element tensors, tensors that start off a 16-byte boundary inside a flat buffer
SHAPES = [(16, 7), (16,), (3,), (1,), (64, 128, 3, 3, 3), (4097,), (8191,), (2, 768, 1, 1), (5, 3)]
DECAY = [i for i, s in enumerate(SHAPES) if len(s) > 1]          # dim() > 1: wd 0.01, lr 2e-3
REST = [i for i, s in enumerate(SHAPES) if len(s) <= 1]          # the rest:  wd 0,    lr 1e-3
BASE = dict(betas=(0.9, 0.999), eps=1e-8)


def ref_groups(lr=(2e-3, 1e-3), betas=(0.9, 0.999), wd=(0.01, 0.0)):
    return [dict(idx=DECAY, lr=lr[0], betas=betas, eps=1e-8, weight_decay=wd[0]),
            dict(idx=REST, lr=lr[1], betas=betas, eps=1e-8, weight_decay=wd[1])]


@functools.lru_cache(maxsize=None)
def inputs(scale, steps, seed=11):
    """(parameters, [gradients per step]) as CPU tensors, computed once and never written"""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g) for s in SHAPES]
    gs = [[torch.randn(s, generator=g) * scale for s in SHAPES] for _ in range(steps)]
    return ps, gs


@functools.lru_cache(maxsize=None)
def reference(scale, steps):
    """the float64 run and the bars for the two standard groups"""
    ps, gs = inputs(scale, steps)
    return reference_for(ps, gs, lambda s: ref_groups())


def reference_for(ps, gs, groups_fn):
    np_p = [p.numpy() for p in ps]
    np_g = [[None if x is None else x.numpy() for x in st] for st in gs]
    r64 = R.run(np_p, groups_fn, np_g, MAX_NORM, np.float64)
    r32 = R.run(np_p, groups_fn, np_g, MAX_NORM, np.float32)
    return r64, R.bars(r64, r32)


def place(tensors, flat):
    """device copies: separate tensors, or views of one flat buffer (tensors then start off 16-byte boundaries)"""
    if not flat:
        return [t.to(DEV) for t in tensors]
    buf = torch.empty(sum(t.numel() for t in tensors), device=DEV)
    out, off = [], 0
    for t in tensors:
        out.append(buf[off:off + t.numel()].view_as(t).copy_(t))
        off += t.numel()
    return out


def make(ps, flat, scale_grads=False, lr=(2e-3, 1e-3), wd=(0.01, 0.0), **kw):
    from voxelnet_amd.optim import ClipAdamW
    params = [torch.nn.Parameter(p) for p in place(ps, flat)]
    opt = ClipAdamW([dict(params=[params[i] for i in DECAY], lr=lr[0], weight_decay=wd[0]),
                     dict(params=[params[i] for i in REST], lr=lr[1], weight_decay=wd[1])],
                    max_norm=MAX_NORM, scale_grads=scale_grads, **dict(BASE, **kw))
    return params, opt


def set_grads(params, grads, flat):
    """separate placement: fresh gradient tensors at every step (the chunk table follows the pointers); flat placement:
    the same views of one buffer refilled (the table is reused without a look)"""
    if not flat or params[0].grad is None:
        for p, g in zip(params, place(grads, flat)):
            p.grad = g
    else:
        for p, g in zip(params, grads):
            p.grad.copy_(g)


def state_of(opt, params):
    return {"p": [p.detach() for p in params], "m": [opt.state[p]["exp_avg"] for p in params],
            "v": [opt.state[p]["exp_avg_sq"] for p in params]}


def check(tag, got, want, bar):
    """got: {"p","m","v"} -> tensors; want: -> float64 arrays (or tensors); prints before it asserts"""
    bad = []
    for q in ("p", "m", "v"):
        err = 0.0
        for a, b in zip(got[q], want[q]):
            b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else b
            if b.size:
                err = max(err, float(np.max(np.abs(a.detach().double().cpu().numpy() - b))))
        print(f"{tag} {q}: bar {bar[q]:.3e} observed {err:.3e} ratio {err / bar[q]:.3f}")
        if not err <= bar[q]:
            bad.append((q, err, bar[q]))
    assert not bad, (tag, bad)


def check_norm(tag, got, want):
    rel = abs(float(got) - float(want)) / float(want)
    print(f"{tag} norm: bar 1.000e-06 observed {rel:.3e} (relative)")
    assert rel <= 1e-6, (tag, float(got), float(want))


@pytest.mark.parametrize("scale", [1.0, 1e-4])
@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("scale_grads", [False, True])
def test_six_steps_match_the_float64_restatement(scale, flat, scale_grads):
    ps, gs = inputs(scale, 6)
    r64, bars = reference(scale, 6)
    # guard, on the reference alone: no step sits on the clamp, and the two scales cover its two sides
    for norm, _, _ in r64:
        assert abs(float(norm) - MAX_NORM) > 1e-3 * MAX_NORM
        assert (float(norm) > MAX_NORM) == (scale == 1.0)
    params, opt = make(ps, flat, scale_grads)
    for s in range(6):
        set_grads(params, gs[s], flat)
        before = [p.grad.clone() for p in params]
        total = opt.step()
        tag = f"six_steps[scale={scale} flat={flat} scale_grads={scale_grads}] step {s + 1}"
        check_norm(tag, total, r64[s][0])
        check(tag, state_of(opt, params), r64[s][2], bars[s])
        for i, (p, g0) in enumerate(zip(params, before)):
            if scale_grads:
                torch.testing.assert_close(p.grad.cpu(), torch.from_numpy(r64[s][1][i]).float(), rtol=1e-6, atol=1e-12)
            else:
                assert torch.equal(p.grad, g0)                      # bit-untouched
            assert float(opt.state[p]["step"]) == s + 1 and opt.state[p]["step"].device.type == "cpu"
            assert opt.state[p]["step"].dtype == torch.float32


def test_first_step_is_the_closed_form():
    """t = 1, wd = 0, zero moments: m = (1-b1) g', v = (1-b2) g'^2 and the bias corrections cancel them, so
    dp = -lr * g' / (|g'| + eps) — about -lr * sign(g).  Zero parameters make p itself the step (no rounding of p + dp);
    a second copy of the tensors with random values checks that an element whose gradient is 0 keeps p bit for bit."""
    from voxelnet_amd.optim import ClipAdamW
    ps, gs = inputs(1.0, 1)
    g = torch.Generator().manual_seed(5)
    grads = [x * (torch.rand(x.shape, generator=g) > 0.1) for x in gs[0]]          # ~10 % exact zeros
    lr, eps = 1e-3, 1e-8
    zeros = [torch.nn.Parameter(torch.zeros_like(p, device=DEV)) for p in ps]
    rnd = [torch.nn.Parameter(p.to(DEV)) for p in ps]
    kept = [p.detach().clone() for p in rnd]
    for p, x in zip(zeros + rnd, grads + grads):
        p.grad = x.to(DEV)
    opt = ClipAdamW(zeros + rnd, lr=lr, eps=eps, weight_decay=0.0, max_norm=MAX_NORM)
    opt.step()
    total = np.sqrt(2.0 * sum(float((x.double() ** 2).sum()) for x in grads))
    coef = min(1.0, MAX_NORM / (total + 1e-6))
    assert coef < 0.02                                             # clipped: g' = g * coef
    worst, n_checked, n_zero = 0.0, 0, 0
    for p, q, q0, x in zip(zeros, rnd, kept, grads):
        gp = x.double().numpy() * coef
        want = -lr * gp / (np.abs(gp) + eps)
        got = p.detach().double().cpu().numpy()
        big = np.abs(gp) > 1e-3
        if big.any():
            worst = max(worst, float(np.max(np.abs(got[big] - want[big]) / np.abs(want[big]))))
            assert np.all(np.abs(got[big] + lr * np.sign(gp[big])) <= 2e-5 * lr)          # eps / |g'| <= 1e-5
        n_checked += int(big.sum())
        zero = (x == 0).numpy()
        n_zero += int(zero.sum())
        assert np.array_equal(got[zero], np.zeros(int(zero.sum())))
        assert torch.equal(q.detach().cpu()[torch.from_numpy(zero)], q0.cpu()[torch.from_numpy(zero)])
    print(f"closed_form: bar 1.000e-06 observed {worst:.3e} (relative, {n_checked} elements; {n_zero} zero gradients)")
    assert n_checked > 100000 and n_zero > 10000
    assert worst <= 1e-6


@pytest.mark.parametrize("scale", [1.0, 1e-4])
def test_three_steps_match_torch_on_the_device(scale):
    ps, gs = inputs(scale, 6)
    _, bars = reference(scale, 6)
    params, opt = make(ps, False)
    tp = [torch.nn.Parameter(p.to(DEV)) for p in ps]
    ref = torch.optim.AdamW([dict(params=[tp[i] for i in DECAY], lr=2e-3, weight_decay=0.01),
                             dict(params=[tp[i] for i in REST], lr=1e-3, weight_decay=0.0)], foreach=False, **BASE)
    for s in range(3):
        set_grads(params, gs[s], False)
        set_grads(tp, gs[s], False)
        total = opt.step()
        ref_total = torch.nn.utils.clip_grad_norm_(tp, MAX_NORM)
        ref.step()
        tag = f"vs_torch[scale={scale}] step {s + 1}"
        check_norm(tag, total, ref_total)
        check(tag, state_of(opt, params), state_of(ref, tp), bars[s])


# the transplant tests run on gradients of scale 0.01: norms of about 4.85, under max_norm, so that the clip coefficient is
# exactly 1 on both sides and what is compared is the state that travelled (torch's CPU norm is only good to 1e-6)
T_SCALE = 0.01


def _torch_twin(ps):
    tp = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    opt = torch.optim.AdamW([dict(params=[tp[i] for i in DECAY], lr=2e-3, weight_decay=0.01),
                             dict(params=[tp[i] for i in REST], lr=1e-3, weight_decay=0.0)], foreach=False, **BASE)
    return tp, opt


def test_state_dict_goes_into_torch_adamw():
    ps, gs = inputs(T_SCALE, 4)
    r64, bars = reference(T_SCALE, 4)
    assert all(float(n) < MAX_NORM * (1 - 1e-3) for n, _, _ in r64)
    params, opt = make(ps, True)
    for s in range(3):
        set_grads(params, gs[s], True)
        opt.step()
    tp, ref = _torch_twin(params)
    ref.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert ref.param_groups[0]["max_norm"] == MAX_NORM              # the extra keys ride along
    assert all(float(ref.state[p]["step"]) == 3 for p in tp)
    set_grads(params, gs[3], True)
    opt.step()
    for p, x in zip(tp, gs[3]):
        p.grad = x.clone()
    torch.nn.utils.clip_grad_norm_(tp, MAX_NORM)
    ref.step()
    check("to_torch step 4 (ours vs torch)", state_of(opt, params), state_of(ref, tp), bars[3])
    check("to_torch step 4 (ours vs float64)", state_of(opt, params), r64[3][2], bars[3])


def test_torch_adamw_state_dict_comes_in():
    ps, gs = inputs(T_SCALE, 4)
    r64, bars = reference(T_SCALE, 4)
    tp, ref = _torch_twin(ps)
    for s in range(4):
        if s == 3:
            params, opt = make([p.detach() for p in tp], False)
            opt.load_state_dict(copy.deepcopy(ref.state_dict()))
            assert opt._table is None and opt.param_groups[1]["max_norm"] == MAX_NORM and opt.param_groups[1]["scale_grads"] is False
            assert all(opt.state[p]["exp_avg"].is_cuda and float(opt.state[p]["step"]) == 3 for p in params)
            set_grads(params, gs[3], False)
            opt.step()
        for p, x in zip(tp, gs[s]):
            p.grad = x.clone()
        torch.nn.utils.clip_grad_norm_(tp, MAX_NORM)
        ref.step()
    assert all(float(opt.state[p]["step"]) == 4 for p in params)
    check("from_torch step 4 (ours vs torch)", state_of(opt, params), state_of(ref, tp), bars[3])
    check("from_torch step 4 (ours vs float64)", state_of(opt, params), r64[3][2], bars[3])


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
def test_a_copied_optimizer_steps_like_its_twin(how):
    ps, gs = inputs(1.0, 6)
    params, opt = make(ps, False)
    for s in range(3):
        set_grads(params, gs[s], False)
        opt.step()
    twin = copy.deepcopy(opt) if how == "deepcopy" else pickle.loads(pickle.dumps(opt))
    tparams = [None] * len(SHAPES)
    for idx, g in zip((DECAY, REST), twin.param_groups):
        for i, p in zip(idx, g["params"]):
            tparams[i] = p
    assert all(tp is not p and tp.data_ptr() != p.data_ptr() for tp, p in zip(tparams, params))
    assert twin._table is None
    set_grads(params, gs[3], False)
    set_grads(tparams, gs[3], False)
    n0, n1 = opt.step(), twin.step()
    assert torch.equal(n0, n1)
    a, b = state_of(opt, params), state_of(twin, tparams)
    for q in ("p", "m", "v"):
        assert all(torch.equal(x, y) for x, y in zip(a[q], b[q])), q
    assert all(float(twin.state[p]["step"]) == 4 for p in tparams)


@pytest.mark.parametrize("kind", ["onecycle", "multistep"])
def test_schedulers_are_honoured_without_a_table_rebuild(kind):
    ps, gs = inputs(1.0, 6)
    params, opt = make(ps, True)
    if kind == "onecycle":
        # total_steps 6, pct_start 0.5, cosine: beta1 = 0.95, 0.9, 0.85, 0.875 at the four steps (short decimals, see the
        # module docstring); lr rises from max_lr / 25 to max_lr and turns
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=[4e-3, 2e-3], total_steps=6, pct_start=0.5, cycle_momentum=True,
                                                    base_momentum=0.85, max_momentum=0.95)
    else:
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2, 3], gamma=0.1)
    seen, tables = [], []
    for s in range(4):
        seen.append([(g["lr"], tuple(g["betas"])) for g in opt.param_groups])
        set_grads(params, gs[s], True)
        opt.step()
        sched.step()
        tables.append(opt._table)
    if kind == "onecycle":
        assert [round(h[0][1][0], 12) for h in seen] == [0.95, 0.9, 0.85, 0.875]
        assert seen[0][0][0] == pytest.approx(4e-3 / 25) and seen[2][0][0] == pytest.approx(4e-3) and seen[2][1][0] == pytest.approx(2e-3)
    else:
        assert [h[0][0] for h in seen] == pytest.approx([2e-3, 2e-3, 2e-4, 2e-5])

    def groups_fn(s):
        (lr0, b0), (lr1, b1) = seen[s]
        g = ref_groups(lr=(lr0, lr1))
        g[0]["betas"], g[1]["betas"] = b0, b1
        return g

    r64, bars = reference_for(ps, gs[:4], groups_fn)
    # (the reference is replayed after the fact: compare the final state, and the table that served all four steps)
    check(f"scheduler[{kind}] step 4", state_of(opt, params), r64[3][2], bars[3])
    assert tables[0] is not None and all(t is tables[0] for t in tables)


def test_a_parameter_without_a_gradient_is_skipped():
    from voxelnet_amd import _lib
    from voxelnet_amd.optim import ClipAdamW
    ps, gs = inputs(1.0, 6)
    steps = [list(gs[0]), list(gs[1]), list(gs[2])]
    steps[1][2] = None                                               # params[2] sits out the second step
    r64, bars = reference_for(ps, steps, lambda s: ref_groups())
    params, opt = make(ps, False)
    set_grads(params, steps[0], False)
    opt.step()
    check("skipped step 1", state_of(opt, params), r64[0][2], bars[0])
    kept = [t.clone() for t in (params[2].detach(), opt.state[params[2]]["exp_avg"], opt.state[params[2]]["exp_avg_sq"])]
    for i, p in enumerate(params):
        p.grad = None if i == 2 else steps[1][i].to(DEV)
    total = opt.step()
    check_norm("skipped step 2", total, r64[1][0])                   # nothing of params[2] in the norm
    now = (params[2].detach(), opt.state[params[2]]["exp_avg"], opt.state[params[2]]["exp_avg_sq"])
    assert all(torch.equal(a, b) for a, b in zip(kept, now)) and float(opt.state[params[2]]["step"]) == 1
    assert all(float(opt.state[p]["step"]) == 2 for i, p in enumerate(params) if i != 2)
    check("skipped step 2", state_of(opt, params), r64[1][2], bars[1])
    # back in: its group now holds two step counts (2 and 3) — two hyperparameter slots, three with the other group
    set_grads(params, steps[2], False)
    total = opt.step()
    assert len(opt._slots) == 3 and float(opt.state[params[2]]["step"]) == 2 and float(opt.state[params[0]]["step"]) == 3
    check_norm("skipped step 3", total, r64[2][0])
    check("skipped step 3", state_of(opt, params), r64[2][2], bars[2])
    # nine groups, each one step further than the next: nine (group, step count) combinations, one more than a call carries
    nine = [torch.nn.Parameter(torch.ones(8, device=DEV)) for _ in range(9)]
    many = ClipAdamW([dict(params=[p]) for p in nine], max_norm=MAX_NORM)
    for r in range(8):                                               # up to eight combinations work
        for i, p in enumerate(nine):
            p.grad = torch.ones(8, device=DEV) if i <= r else None
        assert many.step() is not None and len(many._slots) == r + 1
    assert [int(float(many.state[p]["step"])) for p in nine[:8]] == [8, 7, 6, 5, 4, 3, 2, 1] and len(many.state.get(nine[8], {})) == 0
    for p in nine:
        p.grad = torch.ones(8, device=DEV)
    before = [p.detach().clone() for p in nine]
    with pytest.raises(_lib.VoxelnetHipError, match="9 distinct"):
        many.step()
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, nine))


def test_two_runs_are_bit_equal():
    ps, gs = inputs(1.0, 6)
    runs = []
    for _ in range(2):
        params, opt = make(ps, True, scale_grads=True)
        norms = []
        for s in range(3):
            set_grads(params, gs[s], True)
            norms.append(opt.step().clone())
        runs.append((norms, state_of(opt, params), [p.grad for p in params]))
    (n0, s0, g0), (n1, s1, g1) = runs
    assert all(torch.equal(a, b) for a, b in zip(n0, n1))
    for q in ("p", "m", "v"):
        assert all(torch.equal(a, b) for a, b in zip(s0[q], s1[q])), q
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))


def test_train_step_with_clip_adamw_stays_on_the_one_call_path(monkeypatch):
    """Whole detector (the setup of test_gpu_optim.test_train_step_with_fused_tail_matches_torch_tail: Car grid, batch 1,
    bf16, given targets), two consecutive steps: (a) train_step(x, DEV, ClipAdamW) runs vn_net_step + vn_clip_adamw, (b) bit
    for bit what train_step(x, DEV, None) + opt.step() gives, (c) within rtol 1e-5 / atol 1e-8 of the torch tail
    (clip_grad_norm_ + torch.optim.AdamW) after each step — that test's bar for this comparison; the norm within 1e-5 relative.

    The learning rate is the one at which AdamW moves the parameters as far as that test's SGD step does: SGD(0.01) on a
    gradient clipped to norm 5 moves them by 0.01 * 5 = 0.05; AdamW's first step moves every one of the 6,809,392 elements by
    about lr, 2609 * lr in all: lr = 2e-5.

    The second step's gradient is a property of the bf16 network at the parameters the first step left, and that network
    turns last-bit differences between two correct fp32 updates into 1e-4 .. 1e-3 of the next gradient; Adam then makes
    lr-sized steps of opposite sign out of gradients that are rounding noise.  Measured on the MI355X with an element update
    that was within 0.43 of the bars of torch's but not equal to it in the last bit: step 1 norms 881.774109 on both sides
    (equal bit for bit) and parameters at 0.011 of this bar; step 2 norms 339.1069 against 339.0435 (1.9e-4 relative) and
    parameters at 3088 times the bar (lr = 1e-3: step 2 norms 4506.72 against 4502.67).  csrc/optim.hip's element update
    therefore rounds where torch's device kernels round; with it the step 2 norms are equal bit for bit (339.043549) and
    the parameters sit at 0.011 and 0.015 of the bar after the two steps."""
    from voxelnet_amd import _lib, synth
    from voxelnet_amd import model as M
    from voxelnet_amd.config import grid_config
    from voxelnet_amd.optim import ClipAdamW, decay_param_groups
    from voxelnet_amd.voxelize import voxelize_device
    M.set_precision("bf16")
    grid = grid_config("Car")
    frames = synth.workload_frames(1, batch=1, frame0=0)
    feats, coords = [], []
    for b, f in enumerate(frames):
        fb, cb, _ = voxelize_device(torch.from_numpy(f).to(DEV), grid, b, coord_cols=4)
        feats.append(fb)
        coords.append(cb)
    x = (None, None, feats, None, coords, None, None)
    LR = 2e-5
    names = []
    real_call = _lib.call

    def counting_call(name, *args):
        names.append(name)
        return real_call(name, *args)

    results = {}
    for arm in ("inside", "after", "torch"):
        torch.manual_seed(5)
        model = M.RPN3D("Car").to(DEV).train(True)
        params = list(model.parameters())
        h, w = model.rpn_output_shape
        g = torch.Generator().manual_seed(3)
        pos = (torch.rand((1, h, w, 2), generator=g) < 0.02).float().to(DEV)
        neg = (1 - pos) * (torch.rand((1, h, w, 2), generator=g) < 0.9).float().to(DEV)
        tgt = (torch.randn((1, h, w, 14), generator=g) * 0.3).to(DEV)
        groups = decay_param_groups(model, 0.01)
        if arm == "torch":
            opt = torch.optim.AdamW(groups, lr=LR, foreach=False, **BASE)
        else:
            opt = ClipAdamW(groups, lr=LR, max_norm=MAX_NORM, **BASE)
        norms, snaps = [], []
        for _ in range(2):
            for p in params:
                p.grad = None
            if arm == "inside":
                assert model._step_fused_ok("bf16", opt)
                monkeypatch.setattr(_lib, "call", counting_call)
                model.train_step(x, DEV, opt, targets=(pos, neg, tgt))
                monkeypatch.setattr(_lib, "call", real_call)
                norms.append(opt._norm[0].item())
            elif arm == "after":
                model.train_step(x, DEV, None, targets=(pos, neg, tgt))
                norms.append(opt.step().item())
            else:
                out = model(x, DEV, targets=(pos, neg, tgt))
                out[2].backward()
                norms.append(torch.nn.utils.clip_grad_norm_(params, MAX_NORM).item())
                opt.step()
            snaps.append([p.detach().clone() for p in params])
        torch.cuda.synchronize()
        results[arm] = (norms, snaps)
    assert names.count("vn_net_step") == 2 and names.count("vn_clip_adamw") == 2 and "vn_clip_sgd" not in names, names
    (n_in, p_in), (n_af, p_af), (n_t, p_t) = results["inside"], results["after"], results["torch"]
    assert n_in == n_af and all(torch.equal(a, b) for sa, sb in zip(p_in, p_af) for a, b in zip(sa, sb))
    for k, (a, b) in enumerate(zip(n_in, n_t)):
        print(f"train_step step {k + 1} norm: ours {a:.6f} torch {b:.6f} relative {abs(a - b) / b:.3e} (bar 1e-5)")
    for k, (sa, sb) in enumerate(zip(p_in, p_t)):
        worst = max(float(((a - b).abs() / (1e-8 + 1e-5 * b.abs())).max()) for a, b in zip(sa, sb))
        print(f"train_step step {k + 1} parameters vs the torch tail: largest |a - b| / (1e-8 + 1e-5 |b|) = {worst:.4f} (bar 1)")
    for a, b in zip(n_in, n_t):
        assert abs(a - b) <= 1e-5 * b
    for sa, sb in zip(p_in, p_t):
        for a, b in zip(sa, sb):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-8)
