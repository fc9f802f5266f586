"""GPU: the sparse first Conv3d (middle_layer.0: Conv3d 128 -> 64, k 3, stride (2,1,1), pad (1,1,1)) on the directed
occupancy sets of tests/sparse_cases.py, every kernel against an exact-operand float64 oracle.

  (a) vn_active_sites / vn_voxel_index_grid: the list EQUALS the oracle's (conv3d of the occupancy with an all-ones kernel
      > 0, ascending linear order), *count = min(n, cap), nothing is written past cap, the voxel order does not matter.
  (b) the executor's rulebook route (one P GEMM + vn_rulebook_combine) through run_rulebook_first_layer.
  (c) engine.first_layer_forward_sparse: y, BatchNorm statistics, running buffers, the activation.
  (d) vn_conv_wgrad_rows and vn_conv_gather_gemm_rows(out_linear = 1) over the K voxel rows (the stride-2 depth axis as a
      residue-class gather), isolated, against float64 autograd.
  (e) forward + backward glue against oracle.torch_ref.conv_md in float64 with the kernels' ReLU mask.

Bars (each is one the suite already uses for the same kind of quantity):
  bf16-stored outputs   assert_rounded: half a bf16 ulp + 1e-4 rms per element, rel-L2 3e-3.
  fp32 sums             assert_fp32_sum: 2e-5 * sum|terms| per element (the bias is one of the terms of y), rel-L2 1e-4
                        (1e-3 for weight gradients).
  statistics            1e-4 relative (tests/test_gpu_vfe.py's bar for running statistics)
  fp32 activation, (e)  2e-4 of the maximum, max(2e-4, 1e-3) for gamma / beta (test_layer_fwd_bwd)
The bf16 activation of (c) is BatchNorm of a y that was ROUNDED TO bf16 in between.  It is held, by assert_rounded with no
slack, to relu(bn(.)) of the stored y (which the same test pins to y64 at half an ulp) and, element by element, to
relu(bn(y64)) with test_bf16_layer_stages' slack for that rounding: |S| * half an ulp of y + 2e-4 |z|.  assert_rounded's
rel-L2 part cannot be asked of the second comparison on these grids: S = gamma / sigma, and with a handful of active
sites sigma is so small that the rounding of the stored BIAS at the inactive sites, times S, is most of the distance
(batch_seam: 8 of 168 sites active, rel-L2 3.8e-3 from that alone; empty: sigma = 0, S = 316 gamma).

Measured on an MI355X: worst ratio to the bar over all cases, bf16 / fp32 (1.0 = at the bar; a correctly rounded bf16
output sits just below 1 by construction, anything wrong is far above it), and the case that set it:
  (b) rulebook    y 0.992 (k_257) / 0.030 (lattice)            slab sums 0.0081 (batch_seam) / 0.021 (single)
  (c) layer       y 0.992 (k_257) / 0.028 (k_257)              a 0.979 (k_256), from the stored y 0.997 (k_255) / 0.0067 (full_block)
                  mean 0.0019 / 0.0009, invstd 0.0010 / 0.0014, running mean 0.0022 / 0.0009, running var 0.0003 / 0.0004
  (d) backward    dW 0.0065 (k_257) / 0.014 (k_255)            d_vw 0.0041 (full_block) / 0.012 (k_256)
  (e) glue, fp32  weight 0.0019, gamma 0.0006, beta 0.00004, d_vw 0.0064 (all full_block / corners_faces)
The file's 120 tests take 13 s together; the slowest (the k_* backward cases, lattice) 0.8 s each.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_cases as S
from oracle import torch_ref as tr
from test_gpu_bf16_parity import (DEV, EPS, assert_fp32_sum, assert_rounded, assert_rulebook_slab, bf16r, dense_geom,
                                  emulate_fp32_bn, relu_like, rows_to_nchw64, run_rulebook_first_layer, seeded, ulp_bf16)

pytestmark = pytest.mark.gpu
MODES = ("bf16", "fp32")
SENTINEL = -7777
GUARD = 8                       # rows behind every capacity, prefilled with the sentinel
SEED = 8300


# ------------------------------------------------------------------------------------------------ measuring
def margin(group, mode, what, ratio):
    """printed, never asserted: the bars are asserted by the shared helpers"""
    print(f"MARGIN {group} {mode} {what} {ratio:.3g}")


def ratio_rounded(got, ref, extra=None):
    """worst err / bound of assert_rounded"""
    got = got.detach().double().cpu().numpy()
    ref = np.asarray(ref, dtype=np.float64)
    bound = 0.5 * ulp_bf16(np.maximum(np.abs(got), np.abs(ref))) + 1e-4 * (float(np.sqrt(np.mean(ref * ref))) + 1e-30)
    if extra is not None:
        bound = bound + extra
    return float((np.abs(got - ref) / bound).max()) if got.size else 0.0


def ratio_fp32(got, ref, abs_terms):
    """worst err / bound of assert_fp32_sum"""
    got = got.detach().double().cpu().numpy()
    ref = np.asarray(ref, dtype=np.float64)
    bound = 2e-5 * np.asarray(abs_terms, dtype=np.float64) + 1e-12
    return float((np.abs(got - ref) / bound).max()) if got.size else 0.0


def rel_err(a, b):
    a = a.detach().double().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    b = b.detach().double().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-6))


def the_spec():
    from voxelnet_amd.net import layer_table
    return dict(layer_table(2))["middle_layer.0"]


def rows64(t):
    """NCDHW float64 -> (B, D, H, W, C) numpy"""
    return t.detach().permute(0, 2, 3, 4, 1).contiguous().numpy()


# ------------------------------------------------------------------------------------------------ (a) list and index grid
def list_geom(c):
    from voxelnet_amd import _lib
    return dense_geom(_lib, _lib.VN_BF16, c.B, (c.D, c.H, c.W), S.out_dims(c.D, c.H, c.W), S.CIN, S.COUT, S.KERNEL, S.STRIDE,
                      (1, 1, 1), S.PAD, (1, 1, 1))


def active_sites(c, coord_d, cap):
    """-> (list rows incl. the guard rows, the 64 count words) on the CPU; both prefilled with garbage"""
    from voxelnet_amd import _lib, engine as E
    lib = _lib.load()
    g = list_geom(c)
    nbytes = lib.vn_active_sites_workspace_bytes(ctypes.byref(g))
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=DEV)
    lst = torch.full((cap + GUARD, 4), SENTINEL, dtype=torch.int64, device=DEV)
    cnt = torch.full((64,), -12345, dtype=torch.int32, device=DEV)
    _lib.call("vn_active_sites", coord_d.data_ptr(), coord_d.shape[0], ctypes.byref(g), ws.data_ptr(), nbytes, lst.data_ptr(),
              cap, cnt.data_ptr(), E.stream())
    torch.cuda.synchronize()
    return lst.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("case_id", S.ALL_IDS)
def test_active_site_list_equals_the_oracle(case_id):
    c = S.case(case_id)
    sites, _ = S.oracle(case_id)
    n, K = len(sites), len(c.coord)
    coord_d = torch.from_numpy(np.array(c.coord)).to(DEV)
    cap = S.list_cap(c)
    assert n <= cap
    lst, cnt = active_sites(c, coord_d, cap)
    assert cnt[0] == n and (cnt[1:] == -12345).all(), (cnt[0], n)
    assert np.array_equal(lst[:n], sites), "active sites or their order"
    assert (lst[n:] == SENTINEL).all(), "rows at and past *count were written"
    if n > 1:
        for cut in (n - 1, n // 2):
            l2, c2 = active_sites(c, coord_d, cut)
            assert c2[0] == cut, (c2[0], cut, n)
            assert np.array_equal(l2[:cut], sites[:cut]) and (l2[cut:] == SENTINEL).all(), cut
    if K > 1:
        perm = np.random.default_rng(5).permutation(K)
        l3, c3 = active_sites(c, coord_d[torch.from_numpy(perm).to(DEV)].contiguous(), cap)
        assert np.array_equal(l3, lst) and c3[0] == cnt[0]


@pytest.mark.parametrize("case_id", S.ALL_IDS)
def test_voxel_index_grid(case_id):
    from voxelnet_amd import _lib, engine as E
    c = S.case(case_id)
    K = len(c.coord)
    cells = c.B * c.D * c.H * c.W
    want = np.full(cells, -1, dtype=np.int32)
    co = c.coord
    want[((co[:, 0] * c.D + co[:, 1]) * c.H + co[:, 2]) * c.W + co[:, 3]] = np.arange(K, dtype=np.int32)
    outside = np.concatenate([co, np.array([[c.B, c.D, 0, 0]], dtype=np.int64)])     # one more row: b = B, z = D
    for rows in (co, outside):
        coord_d = torch.from_numpy(np.array(rows)).to(DEV)
        grid = torch.full((cells + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        _lib.call("vn_voxel_index_grid", coord_d.data_ptr(), len(rows), c.B, c.D, c.H, c.W, grid.data_ptr(), E.stream())
        got = grid.cpu().numpy()
        assert np.array_equal(got[:cells], want) and (got[cells:] == SENTINEL).all(), len(rows)


# ------------------------------------------------------------------------------------------------ (b) rulebook forward
@functools.lru_cache(maxsize=None)
def rulebook(case_id, mode):
    """one run of the executor's call sequence on the case + its float64 oracle, shared by (b) and (c):
    ref / abs_terms (B, Do, H, W, 64) float64 numpy, bias included"""
    c = S.case(case_id)
    sparse = case_id == "lattice"
    r = run_rulebook_first_layer(mode, c.B, c.D, c.H, c.W, coord=c.coord, seed=SEED, dense_oracle=not sparse)
    sites, _ = S.oracle(case_id)
    b64 = r["bias"].double()
    if sparse:
        # every site has ONE live tap (tests/test_sparse_cases_host.py): y64[site] = bias + x64[v] @ W64[tap], exactly
        vox, tap = S.single_tap(case_id)
        wt = r["w"].double().reshape(64, 128, 27)
        x64 = r["vw"].double()
        shape = tuple(r["y"].t.shape)
        ref = b64.expand(shape).clone().numpy()
        sabs = b64.abs().expand(shape).clone().numpy()
        for t in np.unique(tap):
            sel = np.flatnonzero(tap == t)
            idx = tuple(sites[sel].T)
            xs = x64[torch.from_numpy(vox[sel].copy())]
            ref[idx] += (xs @ wt[:, :, t].T).numpy()
            sabs[idx] += (xs.abs() @ wt[:, :, t].abs().T).numpy()
        r["ref"], r["abs"] = ref, sabs
    else:
        spec = the_spec()
        r["ref"] = rows64(r["y64"])
        r["abs"] = rows64(F.conv3d(r["dense"].abs(), r["w"].double().abs(), b64.abs(), spec.stride, spec.pad))
    r["dense"] = None
    active = np.zeros(r["ref"].shape[:4], dtype=bool)
    active[tuple(sites.T)] = True
    r["active_mask"] = active
    return r


def assert_conv_output(y, r, mode, group, what):
    """the bars of (b) on a conv output tensor (B, Do, H, W, 64) in the mode's stored dtype"""
    if mode == "bf16":
        assert y.dtype == torch.bfloat16
        margin(group, mode, what, ratio_rounded(y, r["ref"]))
        assert_rounded(y, r["ref"], what)
    else:
        assert y.dtype == torch.float32
        margin(group, mode, what, ratio_fp32(y, r["ref"], r["abs"]))
        assert_fp32_sum(y, r["ref"], r["abs"], what)
    stored = r["bias"].to(y.dtype).to(y.device)
    idle = y[torch.from_numpy(~r["active_mask"]).to(y.device)]
    assert torch.equal(idle, stored.expand_as(idle)), what + ": an inactive site does not hold the bias"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case_id", S.GEMM_IDS)
def test_rulebook_forward(case_id, mode):
    c = S.case(case_id)
    r = rulebook(case_id, mode)
    sites, _ = S.oracle(case_id)
    assert r["active"] == len(sites) and r["cap"] == S.list_cap(c)
    assert np.array_equal(r["list"][:len(sites)].cpu().numpy(), sites)
    assert_conv_output(r["y"].t, r, mode, "rulebook", f"{case_id} y")
    yc = torch.from_numpy(r["ref"]).reshape(-1, 64) - r["bias"].double()
    act = torch.from_numpy(r["active_mask"].reshape(-1))
    assert not bool(yc[~act].any())                  # the oracle itself: an inactive site is the bias, exactly
    s = r["slab"].double().sum(0).cpu()
    margin("rulebook", mode, f"{case_id} slab", max(ratio_fp32(s[0], yc.sum(0).numpy(), yc.abs().sum(0).numpy()),
                                                    ratio_fp32(s[1], (yc * yc).sum(0).numpy(), (yc * yc).sum(0).numpy())))
    assert_rulebook_slab(r, yc_rows=yc[act])
    K = len(c.coord)
    if K > 1:       # sparse.hip's fixed summation order: the voxel order is not part of the result
        perm = np.random.default_rng(6).permutation(K)
        r2 = run_rulebook_first_layer(mode, c.B, c.D, c.H, c.W, coord=c.coord, seed=SEED, perm=perm, dense_oracle=False)
        assert torch.equal(r2["y"].t, r["y"].t) and torch.equal(r2["slab"], r["slab"]), "result depends on the voxel order"


# ------------------------------------------------------------------------------------------------ (c) per-layer route, forward
def layer_params():
    gamma = 1.0 + tr._fill((64,), SEED + 10, 0.2)
    beta = tr._fill((64,), SEED + 11, 0.1)
    return gamma, beta


def scattered_rows(c, vw, mode):
    """the scattered voxel grid as the per-layer route reads it: (B, D, H, W, 128) Rows in the mode's activation dtype"""
    from voxelnet_amd import engine as E
    t = torch.zeros((c.B, c.D, c.H, c.W, S.CIN), dtype=E.act_dtype_of(mode), device=DEV)
    co = torch.from_numpy(np.array(c.coord)).to(DEV)
    t[co[:, 0], co[:, 1], co[:, 2], co[:, 3]] = vw.to(DEV).to(t.dtype)
    return E.Rows(t, S.CIN), co


def forward_sparse(case_id, mode, r):
    from voxelnet_amd import engine as E
    c = S.case(case_id)
    gamma, beta = layer_params()
    P = {"weight": r["w"].to(DEV), "bias": r["bias"].to(DEV), "gamma": gamma.to(DEV), "beta": beta.to(DEV)}
    Bf = {"running_mean": torch.zeros(64, device=DEV), "running_var": torch.ones(64, device=DEV)}
    x, co = scattered_rows(c, r["vw"], mode)
    a, st = E.first_layer_forward_sparse(the_spec(), x, co, P, Bf, True, mode)
    torch.cuda.synchronize()
    return a, st, P, Bf, co


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case_id", S.LAYER_IDS)
def test_first_layer_forward_sparse(case_id, mode):
    r = rulebook(case_id, mode)                      # operands + oracle of (b): the same convolution
    a, st, P, Bf, _ = forward_sparse(case_id, mode, r)
    assert_conv_output(st.y.t, r, mode, "layer", f"{case_id} y")
    # ---- statistics over ALL M rows (the inactive ones hold the bias) and the running buffers
    y64 = torch.from_numpy(r["ref"]).reshape(-1, 64)
    M = y64.shape[0]
    m64, v64 = y64.mean(0), y64.var(0, unbiased=False)
    stats = st.stats.detach().cpu().double().view(4, 64)            # mean | invstd | S | beta
    assert torch.isfinite(stats).all()
    gamma, beta = P["gamma"].cpu().double(), P["beta"].cpu().double()
    e = {"mean": rel_err(stats[0], m64), "invstd": rel_err(stats[1], 1.0 / (v64 + EPS).sqrt()),
         "running_mean": rel_err(Bf["running_mean"], 0.1 * m64),
         "running_var": rel_err(Bf["running_var"], 0.9 + 0.1 * v64 * M / (M - 1))}
    for k, v in e.items():
        margin("layer", mode, f"{case_id} {k}", v / 1e-4)
        assert v < 1e-4, (case_id, k, v)
    assert torch.allclose(stats[2], gamma * stats[1], rtol=1e-6) and torch.equal(stats[3], beta)
    # ---- the activation against relu(BN(y64)) with the kernel's statistics
    z64 = stats[2] * (y64 - stats[0]) + stats[3]
    a_ref = torch.relu(z64).reshape(a.t.shape).numpy()
    if mode == "bf16":
        y_k = st.y.t.detach().cpu()
        sf = [stats[i].float() for i in range(4)]
        _, z = emulate_fp32_bn(y_k.float(), sf[0], sf[2], sf[3])    # from the STORED y: no slack
        margin("layer", mode, f"{case_id} a|stored-y", ratio_rounded(a.t, torch.relu(z).double().numpy()))
        assert_rounded(a.t, torch.relu(z).double().numpy(), f"{case_id} a = relu(bn(y)) from the stored y")
        # from y64: y was rounded to bf16 in between (+ |S| * half an ulp of y), z evaluated in fp32 (test_bf16_layer_stages)
        slack = (stats[2].abs() * 0.5 * torch.from_numpy(ulp_bf16(y_k.double().numpy()))).numpy() + \
            2e-4 * np.abs(z64.reshape(a.t.shape).numpy())
        worst = ratio_rounded(a.t, a_ref, extra=slack)
        margin("layer", mode, f"{case_id} a", worst)
        assert worst <= 1.0, (case_id, "a against relu(bn(y64))", worst)
    else:
        err = rel_err(a.t, a_ref)
        margin("layer", mode, f"{case_id} a", err / 2e-4)
        assert err < 2e-4, (case_id, err)
    if case_id == "empty":
        assert torch.equal(st.y.t, P["bias"].to(st.y.t.dtype).expand_as(st.y.t))
        relu_beta = torch.relu(beta).expand(M, 64).reshape(a.t.shape).numpy()
        if mode == "fp32":
            assert rel_err(a.t, relu_beta) < 2e-4
        else:       # variance 0: S = gamma / sqrt(eps) = 316 gamma multiplies the bf16 rounding of the stored bias, nothing else
            y_k = st.y.t.detach().cpu().double()
            by_s = (stats[2].abs() * 0.5 * torch.from_numpy(ulp_bf16(y_k.numpy()))).numpy()
            assert ratio_rounded(a.t, relu_beta, extra=by_s) <= 1.0


# ------------------------------------------------------------------------------------------------ (d) the two backward row-list launches
def backward_operands(c, mode, seed):
    Do, Ho, Wo = S.out_dims(c.D, c.H, c.W)
    K = len(c.coord)
    dy = seeded((c.B, Do, Ho, Wo, 64), seed, 0.5)
    if mode == "bf16":
        return bf16r(dy), bf16r(seeded((K, 128), seed + 1)), bf16r(tr._fill((64, 128, 3, 3, 3), seed + 2, 1.0 / np.sqrt(128 * 27)))
    return dy, relu_like((K, 128), seed + 1, 1), tr._fill((64, 128, 3, 3, 3), seed + 2, 1.0 / np.sqrt(128 * 27))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case_id", S.BACKWARD_IDS)
def test_backward_row_list_launches(case_id, mode):
    from voxelnet_amd import _lib, engine as E
    c = S.case(case_id)
    spec = the_spec()
    K, C, cin, taps = len(c.coord), 64, 128, 27
    dy, vw, w = backward_operands(c, mode, SEED + 20)
    # ---- float64 autograd of conv3d(scatter(vw), W) with upstream dy, and the same on absolute values
    def grads(x, wt, up):
        x, wt = x.requires_grad_(True), wt.requires_grad_(True)
        F.conv3d(x, wt, None, spec.stride, spec.pad).backward(up)
        return wt.grad, x.grad
    up = dy.double().permute(0, 4, 1, 2, 3).contiguous()
    dw64, dx64 = grads(S.scatter64(c, vw), w.double().clone(), up)
    dwabs, dxabs = grads(S.scatter64(c, vw.abs()), w.double().abs(), up.abs())
    co = torch.from_numpy(np.array(c.coord))
    dvw64, dvwabs = (t[co[:, 0], :, co[:, 1], co[:, 2], co[:, 3]] for t in (dx64, dxabs))
    # ---- the geometry and the two launches of engine._first_layer_backward_sparse
    sdt = E.plain_dtype_of(mode)
    dy_r = E.Rows(dy.to(DEV).to(sdt), C)
    vw_rows = vw.to(DEV).to(sdt).contiguous()
    coord_d = co.to(DEV)
    in_dims = (c.D, c.H, c.W)
    neg_pad = tuple(-q for q in spec.pad)
    g = E._geom(c.B, dy_r, in_dims, C, 0, cin, spec.k, (1, 1, 1), (-1, -1, -1), neg_pad, spec.stride, (0, 0, 0, cin))
    dwp = torch.zeros((taps, cin, C), dtype=torch.float32, device=DEV)
    ws, ws_bytes = E.wgrad_workspace(g, 0, K, DEV)
    _lib.call("vn_conv_wgrad_rows", dy_r.ptr(), vw_rows.data_ptr(), dwp.data_ptr(), ctypes.byref(g), coord_d.data_ptr(), K,
              ws.data_ptr(), ws_bytes, E.stream())
    dw = torch.empty((64, 128, 3, 3, 3), dtype=torch.float32, device=DEV)
    _lib.call("vn_unpack_wgrad", dwp.data_ptr(), cin, C, taps, 2, 1, dw.data_ptr(), E.stream())
    wp = E.pack_weight(w.to(DEV), spec, 1, mode)
    d_vw = torch.full((K + GUARD, cin), float(SENTINEL), dtype=torch.float32, device=DEV)
    g2 = E._geom(c.B, dy_r, in_dims, C, 0, cin, spec.k, (1, 1, 1), (-1, -1, -1), neg_pad, spec.stride, (0, 0, 0, cin))
    _lib.call("vn_conv_gather_gemm_rows", dy_r.ptr(), wp.data_ptr(), None, d_vw.data_ptr(), _lib.VN_F32, ctypes.byref(g2),
              coord_d.data_ptr(), K, None, 1, None, E.stream())
    torch.cuda.synchronize()
    margin("backward", mode, f"{case_id} dW", ratio_fp32(dw, dw64.numpy(), dwabs.numpy()))
    margin("backward", mode, f"{case_id} d_vw", ratio_fp32(d_vw[:K], dvw64.numpy(), dvwabs.numpy()))
    assert bool((d_vw[K:] == float(SENTINEL)).all()), "rows past K were written"
    if case_id == "depth_parity":       # row by row: a failure names the depth and its residue class
        for v, (b, z, y, x) in enumerate(c.coord.tolist()):
            assert_fp32_sum(d_vw[v:v + 1], dvw64[v:v + 1].numpy(), dvwabs[v:v + 1].numpy(),
                            f"depth_parity d_vw of the voxel at z = {z} (residue class {z % 2} of the depth gather)")
    assert_fp32_sum(d_vw[:K], dvw64.numpy(), dvwabs.numpy(), f"{case_id} d_vw")
    assert_fp32_sum(dw, dw64.numpy(), dwabs.numpy(), f"{case_id} dW", l2_tol=1e-3)


# ------------------------------------------------------------------------------------------------ (e) the glue, end to end
@pytest.mark.parametrize("case_id", ("full_block", "corners_faces"))
def test_first_layer_sparse_forward_backward_against_conv_md(case_id):
    from voxelnet_amd import engine as E
    mode = "fp32"
    c = S.case(case_id)
    spec = the_spec()
    r = rulebook(case_id, mode)
    a, st, P, Bf, co = forward_sparse(case_id, mode, r)
    up = seeded((c.B, 64) + S.out_dims(c.D, c.H, c.W), SEED + 30)
    da = E.nchw_to_plain_rows(up.to(DEV), E.plain_dtype_of(mode))
    grads, d_vw = E.first_layer_backward_sparse(st, da, P, mode, co, r["vw"].to(DEV).contiguous())
    torch.cuda.synchronize()
    a_k = rows_to_nchw64(a.t, 3)
    sd = {"L.conv.weight": r["w"].double().requires_grad_(True), "L.conv.bias": r["bias"].double().requires_grad_(True),
          "L.batch_norm.weight": P["gamma"].cpu().double().requires_grad_(True),
          "L.batch_norm.bias": P["beta"].cpu().double().requires_grad_(True),
          "L.batch_norm.running_mean": torch.zeros(64, dtype=torch.float64),
          "L.batch_norm.running_var": torch.ones(64, dtype=torch.float64)}
    x64 = S.scatter64(c, r["vw"]).requires_grad_(True)
    yo = tr.conv_md(x64, sd, "L", 3, spec.stride, spec.pad, training=True, relu_mask=(a_k > 0))
    assert rel_err(a_k, yo.detach()) < 2e-4
    yo.backward(up.double())
    cc = torch.from_numpy(np.array(c.coord))
    checks = (("weight", grads["weight"], sd["L.conv.weight"].grad, 2e-4),
              ("gamma", grads["gamma"], sd["L.batch_norm.weight"].grad, max(2e-4, 1e-3)),
              ("beta", grads["beta"], sd["L.batch_norm.bias"].grad, max(2e-4, 1e-3)),
              ("d_vw", d_vw, x64.grad[cc[:, 0], :, cc[:, 1], cc[:, 2], cc[:, 3]], 2e-4))
    for name, got, ref, tol in checks:
        err = rel_err(got, ref)
        margin("glue", mode, f"{case_id} {name}", err / tol)
        assert err < tol, (case_id, name, err)
    assert float(grads["bias"].abs().max()) == 0.0       # a bias in front of a train-mode BatchNorm
