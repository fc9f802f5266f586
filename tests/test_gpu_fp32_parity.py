"""GPU: the fp32 and fp32x3 kernels, stage by stage, against a float64 oracle on EXACTLY the fp32 operands the kernels read
— at the production tile selections, i.e. the rows of tests/test_gpu_bf16_parity.CASES (ConvMD / DeConv2d, model.py:111-199,
layer table model.py:206-254), one N = 16 heads row and the rulebook first layer.

The two modes are separate template instantiations of every MFMA kernel (own LDS layouts, K-chunk widths, wave
arrangements); which one a row runs is asserted through vn_conv_plan_id / vn_conv_wgrad_plan_id in front of the launches
(test shape == production shape == expected) and printed with the figures:

    forward / data gradient (conv.hip)            fp32 (VN_F32)                        fp32x3 (VN_F32X3)
      100  k_conv_patch, 10x16 pixels             launch_patch<2,2,5,16,true>          same, x3 inner loop
      103  k_conv_patch, 6x32 pixels              launch_patch<4,1,3,32,true>          same, x3 inner loop
      123  k_conv_patch2d, 4x16, 3 weight stages  launch_patch2d<2,2,2,16,3,true>      launch_patch2d<4,2,1,16,3,true> (8 waves)
      0 / 1 / 2 / 4  k_gather_gemm 256x64 /       launch_gg<4,1,4,2,true> / <2,2,4,2,true> / <2,2,2,4,true> / <2,2,5,2,true>
                     128x128 / 64x128 / 160x128
    weight gradient (wgrad.hip; no three-tap and no patch form outside bf16)
      22   k_wgrad 64 x 64 channels               launch_wgrad<2,2,true,1>             launch_wgrad<2,2,true,1,4> (8 waves)
      44   k_wgrad 128 x 128 channels             launch_wgrad<4,4,true,1>             launch_wgrad<4,4,true,1,4>
    BatchNorm passes (bn.hip): the VN_F32 branches of load8 / store8; rulebook: OUT_F32 of k_rulebook_combine.

Operands are NOT bf16-representable (asserted: > 90 % of the non-zero elements of x and w differ from their bf16
rounding), otherwise every lo part of an fp32x3 split is zero: x = relu(N(0,1)) * s_c with s_c log-uniform in [1e-2, 10]
per channel and every 7th W column zero, w = torch_ref._fill(., 1/sqrt(fan)) unrounded, da = N(0,1) with every third row
scaled by 1e-2.  Later stages take the kernel-produced tensor of the earlier stage (its y, its stats, its dy); the ReLU
mask is the kernel's own (z > 0 of emulate_fp32_bn).  EVERY element of every output is checked.

Two oracles, float64 torch on the CPU: the EXACT one, and for fp32x3 the EMULATED one = the float64 sum of the three
products hi.hi + lo.hi + hi.lo with hi = bf16(v), lo = bf16(v - hi) (torch.bfloat16 casts; by linearity evaluated as
op(hi + lo, hi) + op(hi, lo)).  r_model = rel-L2 of the emulated against the exact oracle on the case's own operands: a
property of the reference, not of the kernel (~4.5e-6).

Bars (Sigma|terms| = the same operation on |operands| in float64; K = the reduction length of an output element: the taps
that reach it x source channels for y and dx — never more than taps * Cin —, the number of rows M for dW):
  y, dx   fp32:    per element |err| <= 2e-5 Sigma|terms| + 1e-9 vs exact; rel-L2 vs exact <= sqrt(K) 2^-24 (the
                   random-walk growth of a sequential fp32 accumulation: 2.0e-6 at K = 1152, below r_model, so an fp32
                   kernel that ran x3 products fails)
          fp32x3:  per element the same bar vs emulated and (2e-5 + 3 * 2^-18) Sigma|terms| + 1e-9 vs exact (two split
                   residuals and the dropped lo.lo product, each <= 2^-18 of a term); rel-L2 vs exact <= r_model +
                   sqrt(K) 2^-24
  batch statistics (fused slab -> vn_bn_finalize_slab; deconv rows also vn_bn_stats + vn_bn_finalize), d = y64 - bias:
          |mean_k - mean64| <= 2e-5 mean|d|;  |invstd_k / invstd64 - 1| <= 0.5 * 2e-5 (E[d^2] + 2 |E d| E|d|) / (var + eps);
          running_mean / running_var: the same bounds scaled by the momentum
  a = relu(bn(y)): emulate_fp32_bn on the kernel's y and stats: >= 99.99 % bit-identical, the rest within 1 fp32 ulp
  BatchNorm backward, both routes (slab: vn_bn_bwd_reduce_slab -> _finalize_slab -> _apply, the executor's; double atomics:
          vn_bn_bwd_reduce -> _finalize, engine.layer_backward's): dgamma, dbeta and the three coef rows within
          2e-5 Sigma|terms| of the oracle (assert_fp32_sum) and of each other; dy per element against
          c0 dz + c1 d0 + c2 in float64 with the kernel's own coef: |err| <= 4 * 2^-24 (|c0 dz| + |c1 d0| + |c2|)
          (two fmas and one subtraction)
  dW      per element assert_fp32_sum with the Cauchy-Schwarz Sigma|terms| of the bf16 file; rel-L2 <= sqrt(M) 2^-24
          (fp32x3: + r_model)

Mutation check (on a scratch copy, nothing of it committed): see MUTATION below."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as tr
from test_gpu_bf16_parity import (CASES, assert_fp32_sum, assert_rulebook_slab, dense_geom, emulate_fp32_bn, make_spec,
                                  oracle_conv64, plan_ids, relu_like, rows_to_nchw64, run_rulebook_first_layer, seeded)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
MOMENTUM = 0.1
U = 2.0 ** -24                   # unit roundoff of fp32
X3_EXACT = 2e-5 + 3 * 2.0 ** -18    # per-element bar of fp32x3 against the exact oracle, in units of Sigma|terms|
MODES = ("fp32", "fp32x3")

# MUTATION: vn_mfma_x3 (csrc/common.h) without its lo(a).hi(b) product, rebuilt, the fp32x3 tests of this file run once:
MUTATION = """all 16 fp32x3 tests fail, every conv and wgrad row at every conv stage: rel-L2 against the exact oracle y 1.6e-3 ...
1.8e-3, dx 1.6e-3 ... 1.7e-3, dW 1.5e-3 ... 2.0e-3 where the bars (r_model + sqrt(K) 2^-24) are 4.8e-6 ... 2.1e-5; worst
elements 29 ... 142x (y, dx) and 4.8x (dW) their bounds, batch mean / invstd 1.1 ... 8.8x; the BatchNorm-backward checks, which
run no x3 product, stay green.  Unmodified library: fp32 rel-L2 1.4e-7 ... 1.1e-6, fp32x3 = r_model (4.1e-6 ... 4.7e-6) to two
digits; per-row figures in DESIGN.md section 4."""


def vn_dtype(mode):
    from voxelnet_amd import _lib, engine as E
    return E.VN_F32X3 if mode == "fp32x3" else _lib.VN_F32


def expected_ids(case, dtype):
    """(forward, data-gradient, weight-gradient) ids of a CASES row for operands of `dtype`: the bf16 column; for VN_F32 /
    VN_F32X3 the conv ids of the bf16 column and the weight-gradient ids wgrad_plan (csrc/wgrad.hip) leaves outside bf16:
    22 (64 x 64 channel tile) for the 64-channel Conv3d rows, 44 (128 x 128) for every other row"""
    from voxelnet_amd import _lib
    if dtype == _lib.VN_BF16:
        return tuple(case[10])
    return (case[10][0], case[10][1], 22 if (case[2] == 3 and case[3] == 64 and case[4] == 64) else 44)


@pytest.fixture
def x3_flag():
    """"fp32x3" is "fp32" storage plus the operand dtype VN_F32X3 in every conv geometry and in the weight pack (engine.X3)"""
    from voxelnet_amd import engine as E
    yield E.X3
    E.X3["on"] = False


@pytest.fixture(scope="module", autouse=True)
def cpu_threads():
    """the float64 oracles: at most 16 CPU threads"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, n))
    yield
    torch.set_num_threads(n)


def split64(t):
    """fp32 tensor -> (hi, lo) of the fp32x3 split as float64: hi = bf16(v), lo = bf16(v - hi) (v - hi is exact in fp32)"""
    t = t.float()
    hi = t.bfloat16().float()
    lo = (t - hi).bfloat16().float()
    return hi.double(), lo.double()


def frac_not_bf16(t):
    t = t.float()
    nz = t != 0
    return float(((t.bfloat16().float() != t) & nz).sum()) / max(1, int(nz.sum()))


def conv_grads64(dy, x, w, spec, kind, need_x, need_w):
    """float64 (d/dx, d/dw) of oracle_conv64(x, w) for the upstream dy, without evaluating the forward"""
    n = 3 if (spec.dim == 3 and kind != "deconv") else 2
    s, p = (spec.stride, spec.pad) if n == 3 else (spec.stride[1:], spec.pad[1:])
    gi, gw, _ = torch.ops.aten.convolution_backward(dy, x, w, None, list(s), list(p), [1] * n, kind == "deconv", [0] * n, 1,
                                                    [need_x, need_w, False])
    return gi, gw


def rel_l2(got, ref):
    return float((got - ref).norm() / (ref.norm() + 1e-300))


class Report:
    """collects (what, worst err / bound, rel-L2, rel-L2 bar) of every check of a row and asserts them together at the end,
    so that one run shows every figure of a failing row"""

    def __init__(self, name):
        self.name, self.rows, self.failed = name, [], []

    def elements(self, what, got, ref, bound):
        ratio = float(((got - ref).abs() / bound).max())
        self.rows.append((what, ratio, None, None))
        if not ratio <= 1.0:
            self.failed.append(f"{what}: worst element {ratio:.3g}x its bound")
        return ratio

    def l2(self, what, got, ref, bar):
        v = rel_l2(got, ref)
        self.rows.append((what, None, v, bar))
        if not v <= bar:
            self.failed.append(f"{what}: rel-L2 {v:.3e} > {bar:.3e}")
        return v

    def fp32_sum(self, what, got, ref, terms, l2_tol=1e-4):
        got64, ref64 = got.detach().double().cpu(), torch.as_tensor(np.asarray(ref, dtype=np.float64))
        ratio = float(((got64 - ref64).abs() / (2e-5 * torch.as_tensor(np.asarray(terms, dtype=np.float64)) + 1e-12)).max())
        self.rows.append((what, ratio, rel_l2(got64, ref64), l2_tol))
        try:
            assert_fp32_sum(got, ref, terms, self.name + " " + what, l2_tol=l2_tol)
        except AssertionError as e:
            self.failed.append(f"{what}: {e}")

    def require(self, what, ok, detail=""):
        if not ok:
            self.failed.append(f"{what} {detail}")

    def finish(self, head):
        parts = []
        for what, ratio, l2, bar in self.rows:
            s = what
            if ratio is not None:
                s += f" {ratio:.2g}x"
            if l2 is not None:
                s += f" L2 {l2:.1e}/{bar:.1e}"
            parts.append(s)
        print(f"{self.name:14s} {head}: " + " | ".join(parts))
        assert not self.failed, (self.name, head, self.failed)


def reduction_lengths(spec, kind):
    """terms that reach one element of y / of dx: taps that can contribute x source channels, at most taps * Cin"""
    per = 1
    for k, s in zip(spec.k, spec.stride):
        per *= -(-k // s)
    if kind == "deconv":
        ky, kx = per * spec.cin, spec.taps * spec.cout
    else:
        ky, kx = spec.taps * spec.cin, per * spec.cout
    return min(ky, spec.taps * spec.cin), min(kx, spec.taps * spec.cin)


_ORACLE = {}       # one row at a time: the two modes of a row run back to back and share its float64 oracles


def forward_oracle(case, idx):
    name, kind, dim, cin, cout, k, s, p = case[:8]
    if name in _ORACLE:
        return _ORACLE[name]
    _ORACLE.clear()
    B, sp = case[8]
    spec = make_spec(case)
    fan = cin if kind == "deconv" else cin * spec.taps
    wshape = (cin, cout, k, k) if kind == "deconv" else (cout, cin) + (k,) * dim
    w = tr._fill(wshape, 900 + idx, 1.0 / np.sqrt(fan))
    x = relu_like((B, cin) + tuple(sp), 940 + idx, 1)
    x[..., ::7] = 0.0
    assert frac_not_bf16(x) > 0.9 and frac_not_bf16(w) > 0.9, (name, frac_not_bf16(x), frac_not_bf16(w))
    o = {"x": x, "w": w}
    xd, wd = x.double(), w.double()
    o["y64"] = oracle_conv64(xd, wd, spec, kind)                              # without bias
    o["sabs"] = oracle_conv64(xd.abs(), wd.abs(), spec, kind)
    (xh, xl), (wh, wl) = split64(x), split64(w)
    o["yemu"] = oracle_conv64(xh + xl, wh, spec, kind) + oracle_conv64(xh, wl, spec, kind)
    o["r_y"] = rel_l2(o["yemu"], o["y64"])
    _ORACLE[name] = o
    return o


ROWS = [(case, mode) for case in CASES for mode in MODES]


@pytest.mark.parametrize("case,mode", ROWS, ids=[f"{c[0]}-{m}" for c, m in ROWS])
def test_fp32_layer_stages(case, mode, x3_flag):
    from voxelnet_amd import _lib, engine as E
    x3 = mode == "fp32x3"
    x3_flag["on"] = x3
    lib = _lib.load()
    name, kind, dim, cin, cout, k, s, p = case[:8]
    idx = [c[0] for c in CASES].index(name)
    (B, sp), (Bp, spp) = case[8], case[9]
    spec = make_spec(case)
    in_dims = (1,) + tuple(sp) if dim == 2 else tuple(sp)
    # ---- the kernels this size runs are the kernels production runs in this mode
    dt = vn_dtype(mode)
    ids = plan_ids(_lib, spec, B, in_dims, dt)
    ids_prod = plan_ids(_lib, spec, Bp, (1,) + tuple(spp) if dim == 2 else tuple(spp), dt)
    assert ids == ids_prod == expected_ids(case, dt), (name, mode, ids, ids_prod)
    rep = Report(name)
    dev = torch.device(DEV)
    taps = spec.taps
    o = forward_oracle(case, idx)
    x, w, y64 = o["x"], o["w"], o["y64"]
    ky, kx = reduction_lengths(spec, kind)
    bias = tr._fill((cout,), 910 + idx, 0.1)
    gamma = 1.0 + tr._fill((cout,), 920 + idx, 0.2)
    beta = tr._fill((cout,), 930 + idx, 0.1)
    P = {"weight": w.to(dev), "bias": bias.to(dev), "gamma": gamma.to(dev), "beta": beta.to(dev)}
    Bf = {"running_mean": torch.zeros(cout, device=dev), "running_var": torch.ones(cout, device=dev)}
    xr = E.nchw_to_rows(x.to(dev), mode)
    assert xr.t.dtype == torch.float32 and torch.equal(rows_to_nchw64(xr.t, dim).float(), x)

    # ================= stage 1: convolution forward + fused statistics + BatchNorm apply =================
    a, st = E.layer_forward(spec, xr, P, Bf, True, mode)
    assert st.x3 == x3 and st.y.t.dtype == torch.float32 and a.t.dtype == torch.float32
    red = (0, 2, 3, 4) if dim == 3 else (0, 2, 3)
    shp = (1, cout, 1, 1, 1) if dim == 3 else (1, cout, 1, 1)
    b64 = bias.double().view(shp)
    y_k = rows_to_nchw64(st.y.t, dim)
    if x3:
        rep.elements("y~emu", y_k, o["yemu"] + b64, 2e-5 * o["sabs"] + 1e-9)
        rep.elements("y", y_k, y64 + b64, X3_EXACT * o["sabs"] + 1e-9)
    else:
        rep.elements("y", y_k, y64 + b64, 2e-5 * o["sabs"] + 1e-9)
    rep.l2("y", y_k - b64, y64, (o["r_y"] if x3 else 0.0) + np.sqrt(ky) * U)
    # batch statistics against the oracle's
    n = y64[:, 0].numel()
    Ed, Ead, Ed2 = y64.mean(dim=red), y64.abs().mean(dim=red), (y64 * y64).mean(dim=red)
    v64 = y64.var(dim=red, unbiased=False)
    mean_bound = 2e-5 * Ead
    var_bound = 2e-5 * (Ed2 + 2 * Ed.abs() * Ead)
    inv_bound = 0.5 * var_bound / (v64 + EPS)
    m64 = Ed + bias.double()
    rm64, rv64 = MOMENTUM * m64, (1 - MOMENTUM) + MOMENTUM * v64 * n / (n - 1)

    def check_stats(tag, stats_t, rmean, rvar):
        sk = stats_t.detach().cpu().double().view(4, cout)                  # mean | invstd | S | beta
        rep.elements(tag + "mean", sk[0], m64, mean_bound)
        rep.elements(tag + "invstd", sk[1] * (v64 + EPS).sqrt(), torch.ones_like(v64), inv_bound)
        rep.elements(tag + "run_mean", rmean.cpu().double(), rm64, MOMENTUM * mean_bound)
        rep.elements(tag + "run_var", rvar.cpu().double(), rv64, MOMENTUM * var_bound * n / (n - 1))
        rep.require(tag + "S = gamma * invstd", torch.allclose(sk[2], gamma.double() * sk[1], rtol=2 * U, atol=0))
        rep.require(tag + "beta", torch.equal(sk[3].float(), beta))

    check_stats("", st.stats, Bf["running_mean"], Bf["running_var"])
    M, C = st.y.M, cout
    if kind == "deconv":
        # the two-pass route of a ConvTranspose2d's statistics: vn_bn_stats over the kernel's y, then vn_bn_finalize
        sums = torch.zeros(2 * C, dtype=torch.float64, device=dev)
        stats2 = torch.empty(4 * C, dtype=torch.float32, device=dev)
        rm2, rv2 = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        _lib.call("vn_bn_stats", st.y.ptr(), _lib.VN_F32, M, C, st.y.row_stride(), 1, P["bias"].data_ptr(), sums.data_ptr(),
                  E.stream())
        _lib.call("vn_bn_finalize", sums.data_ptr(), M, C, 1, P["bias"].data_ptr(), P["gamma"].data_ptr(), P["beta"].data_ptr(),
                  rm2.data_ptr(), rv2.data_ptr(), 1, MOMENTUM, EPS, stats2.data_ptr(), E.stream())
        check_stats("2pass ", stats2, rm2, rv2)
    # BatchNorm + ReLU of the kernel's own y with the kernel's own statistics: the same fp32 formula
    stats = st.stats.detach().cpu().view(4, cout)
    sf = [stats[i].view(shp) for i in range(4)]
    d0, z = emulate_fp32_bn(y_k.float(), sf[0], sf[2], sf[3])
    a_k = rows_to_nchw64(a.t, dim).float().numpy()
    a_ref = torch.relu(z).numpy()
    same = float((a_k.view(np.int32) == a_ref.view(np.int32)).mean())
    ulp = np.spacing(np.maximum(np.abs(a_k), np.abs(a_ref)))
    rep.rows.append((f"a bit-identical {same:.6f}", None, None, None))
    rep.require("a = relu(bn(y))", same >= 0.9999 and bool((np.abs(a_k.astype(np.float64) - a_ref) <= ulp).all()), f"{same}")

    # ================= stage 2: BatchNorm backward, both routes =================
    od = st.out_dims
    da_rows = seeded((M, C), 950 + idx)
    da_rows[::3] *= 1e-2
    dar = E.Rows(da_rows.view((B,) + tuple(od) + (C,)).to(dev), C)
    nslab = lib.vn_bn_bwd_slab_rows(M, C)
    slab = torch.empty((nslab, 2, C), dtype=torch.float32, device=dev)
    out_s = [torch.empty(3 * C, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev),
             torch.empty(C, dtype=torch.float32, device=dev)]            # coef | dgamma | dbeta
    out_a = [torch.empty_like(t) for t in out_s]
    dy = E.new_rows(B, od, C, torch.float32, False, dev)
    f32 = _lib.VN_F32
    _lib.call("vn_bn_bwd_reduce_slab", dar.ptr(), f32, dar.row_stride(), st.y.ptr(), f32, st.y.row_stride(), M, C,
              st.stats.data_ptr(), 1, slab.data_ptr(), E.stream())
    _lib.call("vn_bn_bwd_finalize_slab", slab.data_ptr(), nslab, M, C, P["gamma"].data_ptr(), st.stats.data_ptr(),
              out_s[0].data_ptr(), out_s[1].data_ptr(), out_s[2].data_ptr(), E.stream())
    _lib.call("vn_bn_bwd_apply", dar.ptr(), f32, dar.row_stride(), st.y.ptr(), f32, st.y.row_stride(), M, C,
              st.stats.data_ptr(), out_s[0].data_ptr(), 1, dy.ptr(), f32, dy.row_stride(), 0, E.stream())
    sums = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    _lib.call("vn_bn_bwd_reduce", dar.ptr(), f32, dar.row_stride(), st.y.ptr(), f32, st.y.row_stride(), M, C,
              st.stats.data_ptr(), 1, sums.data_ptr(), E.stream())
    _lib.call("vn_bn_bwd_finalize", sums.data_ptr(), M, C, 1, P["gamma"].data_ptr(), st.stats.data_ptr(), out_a[0].data_ptr(),
              out_a[1].data_ptr(), out_a[2].data_ptr(), E.stream())
    da64 = rows_to_nchw64(dar.t, dim)
    dz = da64 * (z > 0).double()                                          # the kernels' mask: z > 0 in fp32
    S64, inv64 = sf[2].double(), sf[1].double()
    xh = d0.double() * inv64
    s1, s2 = dz.sum(dim=red), (dz * xh).sum(dim=red)
    t1, t2 = dz.abs().sum(dim=red), (dz * xh).abs().sum(dim=red)
    Sc, ic = S64.reshape(-1), inv64.reshape(-1)
    coef_ref = torch.cat([Sc, -Sc * ic * s2 / M, -Sc * s1 / M])
    coef_terms = torch.cat([Sc.abs(), (Sc * ic).abs() * t2 / M, Sc.abs() * t1 / M])
    for tag, (coef, dgam, dbet) in (("slab ", out_s), ("atomic ", out_a)):
        rep.fp32_sum(tag + "dbeta", dbet, s1.numpy(), t1.numpy())
        rep.fp32_sum(tag + "dgamma", dgam, s2.numpy(), t2.numpy())
        rep.fp32_sum(tag + "coef", coef, coef_ref.numpy(), coef_terms.numpy())
    rep.elements("slab~atomic dbeta", out_s[2].double().cpu(), out_a[2].double().cpu(), 2e-5 * t1 + 1e-12)
    rep.elements("slab~atomic dgamma", out_s[1].double().cpu(), out_a[1].double().cpu(), 2e-5 * t2 + 1e-12)
    rep.elements("slab~atomic coef", out_s[0].double().cpu(), out_a[0].double().cpu(), 2e-5 * coef_terms + 1e-12)
    ck = [out_s[0].detach().cpu().double()[i * C:(i + 1) * C].view(shp) for i in range(3)]
    dy_k = rows_to_nchw64(dy.t, dim)
    q0, q1 = ck[0] * dz, ck[1] * d0.double()
    rep.elements("dy", dy_k, q0 + q1 + ck[2], 4 * U * (q0.abs() + q1.abs() + ck[2].abs()) + 1e-300)
    del q0, q1, dz, xh, da64

    # ================= stages 3 + 4: weight gradient and data gradient from the kernel's dy =================
    xd, wd = x.double(), w.double()
    dx64, dw64 = conv_grads64(dy_k, xd, wd, spec, kind, True, True)
    dxabs, _ = conv_grads64(dy_k.abs(), xd, wd.abs(), spec, kind, True, False)
    r_w = r_x = 0.0
    if x3:
        (dh, dl), (xh_, xl_), (wh, wl) = split64(dy_k), split64(x), split64(w)
        dwemu = conv_grads64(dh, xh_ + xl_, wd, spec, kind, False, True)[1] + conv_grads64(dl, xh_, wd, spec, kind, False, True)[1]
        dxemu = conv_grads64(dh + dl, xd, wh, spec, kind, True, False)[0] + conv_grads64(dh, xd, wl, spec, kind, True, False)[0]
        r_w, r_x = rel_l2(dwemu, dw64), rel_l2(dxemu, dx64)
    one = (1, 1, 1)
    dw = torch.empty_like(P["weight"])
    chunks = ctypes.c_int32(0)
    if spec.transposed:
        g = E._geom(B, dy, st.in_dims, cout, 0, cin, spec.k, spec.stride, one, spec.pad, one, xr.strides)
        srcp, rowp, un, Mw = dy.ptr(), xr.ptr(), (cin, cout), xr.M
    else:
        g = E._geom(B, xr, od, cin, 0, cout, spec.k, spec.stride, one, spec.pad, one, dy.strides)
        srcp, rowp, un, Mw = xr.ptr(), dy.ptr(), (cout, cin), M
    assert g.dtype == dt and lib.vn_conv_wgrad_plan_id(ctypes.byref(g), 0, 0) == ids[2]
    ws, ws_bytes = E.wgrad_workspace(g, 0, 0, dev)
    _lib.call("vn_conv_wgrad_partials", srcp, rowp, ctypes.byref(g), 0, None, 0, ws.data_ptr(), ws_bytes,
              ctypes.byref(chunks), E.stream())
    jobs = (_lib.VnUnpackJob * 1)()
    jobs[0] = _lib.VnUnpackJob(ws.data_ptr(), dw.data_ptr(), un[0], un[1], taps, 0, 1, chunks.value, taps * cin * cout)
    _lib.call("vn_unpack_wgrads_batch", jobs, 1, E.stream())
    # sum|terms| of a weight-gradient element ~ sum_m |x||dy| <= sqrt(sum x^2 sum dy^2): the Cauchy-Schwarz bound
    xs, ds = float(np.sqrt((xd ** 2).sum() / cin)), float(np.sqrt((dy_k ** 2).sum() / cout))
    rep.fp32_sum("dW", dw, dw64.numpy(), np.full(tuple(dw64.shape), xs * ds), l2_tol=r_w + np.sqrt(Mw) * U)
    dx = E.Rows(torch.empty((B,) + tuple(st.in_dims) + (cin,), dtype=torch.float32, device=dev), cin)
    wp = E.pack_weight(P["weight"], spec, 3 if spec.transposed else 1, mode)
    neg = tuple(-q for q in spec.pad)
    if spec.transposed:
        gd = E.gather_geometry(dy, dx, spec.k, cout, cin, spec.stride, one, spec.pad, one, st.in_dims)
        E.gather_gemm(dy, wp, None, dx, spec.k, cout, cin, spec.stride, one, spec.pad, one, st.in_dims)
    else:
        gd = E.gather_geometry(dy, dx, spec.k, cout, cin, one, (-1, -1, -1), neg, spec.stride, st.in_dims)
        E.gather_gemm(dy, wp, None, dx, spec.k, cout, cin, one, (-1, -1, -1), neg, spec.stride, st.in_dims)
    assert gd.dtype == dt and lib.vn_conv_plan_id(ctypes.byref(gd)) == ids[1]
    dx_k = rows_to_nchw64(dx.t, dim)
    if x3:
        rep.elements("dx~emu", dx_k, dxemu, 2e-5 * dxabs + 1e-9)
        rep.elements("dx", dx_k, dx64, X3_EXACT * dxabs + 1e-9)
    else:
        rep.elements("dx", dx_k, dx64, 2e-5 * dxabs + 1e-9)
    rep.l2("dx", dx_k, dx64, r_x + np.sqrt(kx) * U)
    rep.finish(f"{mode} kernels {ids} r_model y/dW/dx {o['r_y']:.1e}/{r_w:.1e}/{r_x:.1e}")


_HEADS = {}


@pytest.mark.parametrize("mode", MODES)
def test_fp32_heads_row(mode, x3_flag):
    """prob_conv + reg_conv (model.py:253-254, 276-281) as the N = 16 GEMM over the 768-channel concat: B = 1, 37 x 45 =
    1665 rows = 6 tiles of 256 + 129 (k_gather_gemm 256 x 64, plan 0, as the full 2 x 200 x 176 map), its data gradient
    (16 -> 768), weight gradient and bias gradient through engine.layer_backward"""
    from voxelnet_amd import _lib, engine as E
    from voxelnet_amd.net import HEADS
    x3 = mode == "fp32x3"
    x3_flag["on"] = x3
    lib = _lib.load()
    dev = torch.device(DEV)
    dt = vn_dtype(mode)
    B, H, W = 1, 37, 45
    one, zero = (1, 1, 1), (0, 0, 0)
    fwd = [lib.vn_conv_plan_id(ctypes.byref(dense_geom(_lib, dt, b, (1, h, w_), (1, h, w_), 768, 16, one, one, one, zero, one)))
           for b, h, w_ in ((B, H, W), (2, 200, 176))]
    assert fwd == [0, 0], fwd
    if not _HEADS:
        x = relu_like((B, 768, H, W), 7101, 1)
        x[..., ::7] = 0.0
        w = tr._fill((16, 768, 1, 1), 7102, 1.0 / np.sqrt(768))
        assert frac_not_bf16(x) > 0.9 and frac_not_bf16(w) > 0.9
        xd, wd = x.double(), w.double()
        (xh, xl), (wh, wl) = split64(x), split64(w)
        _HEADS.update(x=x, w=w, y64=F.conv2d(xd, wd), sabs=F.conv2d(xd.abs(), wd.abs()),
                      yemu=F.conv2d(xh + xl, wh) + F.conv2d(xh, wl))
    o = _HEADS
    x, w, y64 = o["x"], o["w"], o["y64"]
    r_y = rel_l2(o["yemu"], y64)
    b = tr._fill((16,), 7103, 0.1)
    b64 = b.double().view(1, 16, 1, 1)
    P = {"weight": w.to(dev), "bias": b.to(dev)}
    xr = E.nchw_to_rows(x.to(dev), mode)
    y, st = E.layer_forward(HEADS, xr, P, None, True, mode, y_dtype=torch.float32)
    rep = Report("heads")
    y_k = rows_to_nchw64(y.t, 2)
    if x3:
        rep.elements("y~emu", y_k, o["yemu"] + b64, 2e-5 * o["sabs"] + 1e-9)
        rep.elements("y", y_k, y64 + b64, X3_EXACT * o["sabs"] + 1e-9)
    else:
        rep.elements("y", y_k, y64 + b64, 2e-5 * o["sabs"] + 1e-9)
    rep.l2("y", y_k - b64, y64, (r_y if x3 else 0.0) + np.sqrt(768) * U)
    M = B * H * W
    dy_rows = seeded((M, 16), 7104, 1e-2)
    dy_rows[::3] *= 1e-2
    dyv = dy_rows.view(B, H, W, 16).permute(0, 3, 1, 2).contiguous()
    dyr = E.nchw_to_rows(dyv.to(dev), mode)
    grads, dx = E.layer_backward(st, dyr, P, mode)
    dyd, xd, wd = dyv.double(), x.double(), w.double()
    dx64, dw64 = conv_grads64(dyd, xd, wd, HEADS, "conv", True, True)
    dxabs = conv_grads64(dyd.abs(), xd, wd.abs(), HEADS, "conv", True, False)[0]
    r_w = r_x = 0.0
    dx_k = rows_to_nchw64(dx.t, 2)
    if x3:
        (dh, dl), (xh, xl), (wh, wl) = split64(dyv), split64(x), split64(w)
        dwemu = conv_grads64(dh, xh + xl, wd, HEADS, "conv", False, True)[1] + conv_grads64(dl, xh, wd, HEADS, "conv", False, True)[1]
        dxemu = conv_grads64(dh + dl, xd, wh, HEADS, "conv", True, False)[0] + conv_grads64(dh, xd, wl, HEADS, "conv", True, False)[0]
        r_w, r_x = rel_l2(dwemu, dw64), rel_l2(dxemu, dx64)
        rep.elements("dx~emu", dx_k, dxemu, 2e-5 * dxabs + 1e-9)
        rep.elements("dx", dx_k, dx64, X3_EXACT * dxabs + 1e-9)
    else:
        rep.elements("dx", dx_k, dx64, 2e-5 * dxabs + 1e-9)
    rep.l2("dx", dx_k, dx64, r_x + np.sqrt(16) * U)
    xs, ds = float(np.sqrt((xd ** 2).sum() / 768)), float(np.sqrt((dyd ** 2).sum() / 16))
    rep.fp32_sum("dW", grads["weight"], dw64.numpy(), np.full((16, 768, 1, 1), xs * ds), l2_tol=r_w + np.sqrt(M) * U)
    rep.fp32_sum("db", grads["bias"], dyd.sum(dim=(0, 2, 3)).numpy(), dyd.abs().sum(dim=(0, 2, 3)).numpy())
    rep.finish(f"{mode} forward kernel {fwd[0]} r_model y/dW/dx {r_y:.1e}/{r_w:.1e}/{r_x:.1e}")


@pytest.mark.parametrize("mode", MODES)
def test_fp32_rulebook_first_layer(mode, x3_flag):
    """middle_layer.0 (model.py:207) as the executor runs it in the fp32 modes: the P GEMM (voxel rows x packed weights, Cr =
    27 * 64) with VN_F32 / VN_F32X3 operands, vn_rulebook_combine with VN_F32 output, on the coordinates of the bf16 test
    (B = 2, 10 x 134 x 140, K = 3000), against conv3d of the scattered grid in float64: y with the stage-1 bars (K = 128
    channels x the most voxels in reach of one output site), the slab sums within the fp32-sum bound"""
    from voxelnet_amd.net import layer_table
    x3 = mode == "fp32x3"
    x3_flag["on"] = x3
    r = run_rulebook_first_layer(mode)
    spec = dict(layer_table(2))["middle_layer.0"]
    y = r["y"]
    assert y.t.dtype == torch.float32
    assert frac_not_bf16(r["vw"]) > 0.9 and frac_not_bf16(r["w"]) > 0.9
    dense, wd = r["dense"], r["w"].double()
    b64 = r["bias"].double().view(1, 64, 1, 1, 1)
    y64 = r["y64"] - b64
    sabs = F.conv3d(dense.abs(), wd.abs(), None, spec.stride, spec.pad)
    occ = (dense.abs().sum(dim=1, keepdim=True) > 0).double()
    reach = int(F.conv3d(occ, torch.ones((1, 1, 3, 3, 3), dtype=torch.float64), None, spec.stride, spec.pad).max())
    K = 128 * reach
    y_k = rows_to_nchw64(y.t, 3)
    rep = Report("rulebook")
    r_y = 0.0
    if x3:
        (xh, xl), (wh, wl) = split64(dense), split64(r["w"])
        yemu = F.conv3d(xh + xl, wh, None, spec.stride, spec.pad) + F.conv3d(xh, wl, None, spec.stride, spec.pad)
        r_y = rel_l2(yemu, y64)
        rep.elements("y~emu", y_k, yemu + b64, 2e-5 * sabs + 1e-9)
        rep.elements("y", y_k, y64 + b64, X3_EXACT * sabs + 1e-9)
    else:
        rep.elements("y", y_k, y64 + b64, 2e-5 * sabs + 1e-9)
    rep.l2("y", y_k - b64, y64, r_y + np.sqrt(K) * U)
    try:
        assert_rulebook_slab(r)
    except AssertionError as e:
        rep.failed.append(f"slab sums: {e}")
    rep.finish(f"{mode} P GEMM kernel {r['gemm_plan']}, K = 128 x {reach}, active sites {r['active']} of {r['M']}, r_model {r_y:.1e}")
