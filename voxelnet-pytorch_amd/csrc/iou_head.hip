// IoU-aware confidence head of the RPN: a second Conv2d(768, 2, 1) on the concatenation gives one logit per
// anchor (site s, rotation a) in the site layout of prob — z[b, a, s], q = sigmoid(z) — trained to predict the IoU of the
// box the anchor's regression channels decode to with the box its target decodes to; the decode ranks by p^(1-alpha) q^alpha.
//   t[b, a, s] = clamp(IoU(decode(delta[b, 7a..7a+6, s], A_n), decode(targets[b, s, 7a..7a+6], A_n)), 0, 1),  n = 2s + a
//                rpn_common.h's vn_iou_pair_value: the value iou_loss.hip differentiates, an invalid pair scores 0.
//                A CONSTANT: nothing here writes a gradient for delta.
//   bce(z, t)  = max(z, 0) - z t + log1p(exp(-|z|))
//   L          = sum_b (1 / P_b) sum over positives of m bce(z, t),   P_b = max(1, sum pos[b]),  m = pos[b, s, a]
//   mae        = sum m |q - t| / max(1, sum m)
//   d_z        = (m / P_b) (q - t) at the positives, +0.0 elsewhere (what vn_dir_head_bwd skips)
//   p'         = (float)(pow((double)p, 1 - alpha) * pow(q, alpha))
// The loss is rpn_common.h's site-term scaffold around k_iou_head_loss (one thread per site, work where m != 0 only, float64,
// no atomics).  The head's own forward and backward are dir_head.hip's vn_dir_head_fwd / _bwd, which do not care what the
// two logits mean; vn_site_heads_fwd here is that forward for TWO such heads (4 outputs) in one read of the concatenation.
#include <cmath>
#include "rpn_common.h"

namespace {

static_assert(DH_THREADS == VN_SITE_THREADS, "k_iou_head_loss is launched with the scaffold's workgroup count");

template <bool BWD>
__global__ void __launch_bounds__(DH_THREADS) k_iou_head_loss(const float *__restrict__ logits, const float *__restrict__ delta,
                                                             const float *__restrict__ pos, const float *__restrict__ tgt,
                                                             const double *__restrict__ anchors, const double *__restrict__ part,
                                                             int B, int64_t hw, int metric, double *__restrict__ slab /* [blocks][3] */,
                                                             float *__restrict__ d_logits, float *__restrict__ iou_target) {
    VN_PRIO_MAIN();
    const int64_t sites = hw * B;
    const int64_t site = (int64_t)blockIdx.x * DH_THREADS + threadIdx.x;
    double s_loss = 0.0, s_abs = 0.0, s_m = 0.0;
    if (site < sites) {
        const int b = (int)(site / hw);
        const int64_t yx = site - (int64_t)b * hw;
        const float2 ps = *reinterpret_cast<const float2 *>(pos + site * 2);
#pragma unroll 1
        for (int a = 0; a < 2; ++a) {
            const float m = a ? ps.y : ps.x;
            const int64_t at = ((int64_t)b * 2 + a) * hw + yx;
            float out = 0.f, t_out = 0.f;
            if (m != 0.f) {
                double dp[7], dg[7], A[7], P[7], G[7], diag, S, V, ib, i3;
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    dp[j] = (double)delta[((int64_t)b * 14 + a * 7 + j) * hw + yx];
                    dg[j] = (double)tgt[site * 14 + a * 7 + j];
                    A[j] = anchors[(yx * 2 + a) * 7 + j];
                }
                vn_iou_pair_value(dp, dg, A, metric, diag, P, G, S, V, ib, i3);          // (an invalid pair: ib = i3 = 0)
                const double t = fmin(fmax(metric == VN_IOU_3D ? i3 : ib, 0.0), 1.0);
                const double z = (double)logits[at];
                const double q = 1.0 / (1.0 + exp(-z));
                const double wgt = (double)m / fmax(vn_pos_total(part, b), 1.0);
                s_loss += wgt * (fmax(z, 0.0) - z * t + log1p(exp(-fabs(z))));
                s_abs += (double)m * fabs(q - t);
                s_m += (double)m;
                t_out = (float)t;
                if (BWD) out = (float)(wgt * (q - t));
            }
            if (BWD) d_logits[at] = out;
            if (iou_target) iou_target[at] = t_out;
        }
    }
    const double t = vn_block_sum3<DH_THREADS>(s_loss, s_abs, s_m);
    if (threadIdx.x < 3) slab[(int64_t)blockIdx.x * 3 + threadIdx.x] = t;
}

// alpha == 0 copies p (its bits, a NaN's payload included); otherwise both powers are float64 and the product is rounded once
__global__ void __launch_bounds__(DH_THREADS) k_iou_rectify(const float *__restrict__ probs, const float *__restrict__ z, int64_t n,
                                                           double alpha, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * DH_THREADS + threadIdx.x;
    if (i >= n) return;
    const float p = probs[i];
    if (alpha == 0.0) {
        out[i] = p;
        return;
    }
    const double q = 1.0 / (1.0 + exp(-(double)z[i]));
    out[i] = (float)(pow((double)p, 1.0 - alpha) * pow(q, alpha));
}

// k_dir_head_fwd (dir_head.hip) for NOUT outputs in one read of the rows: the lane's 24 x NOUT weights in registers, per
// output the same 24 FMAs in channel order and the same butterfly over the half-wave's 32 lanes, so output c has the bits
// vn_dir_head_fwd gives for weight row c.  logits[b][c][s], c < NOUT.
template <int DT, int NOUT>
__global__ void __launch_bounds__(DH_THREADS) k_site_heads_fwd(const void *__restrict__ cat_, int64_t stride, const float *__restrict__ w,
                                                              const float *__restrict__ bias, int64_t M, int64_t S,
                                                              float *__restrict__ logits) {
    VN_PRIO_MAIN();
    typedef DhRow<DT> R;
    const typename R::elem_t *cat = static_cast<const typename R::elem_t *>(cat_);
    __shared__ float stage[NOUT][DH_TILE];
    const int lane = threadIdx.x & 31, half = threadIdx.x >> 5;
    float wk[NOUT][R::NLOAD][R::PER], bk[NOUT];
#pragma unroll
    for (int c = 0; c < NOUT; ++c) {
#pragma unroll
        for (int j = 0; j < R::NLOAD; ++j)
#pragma unroll
            for (int e = 0; e < R::PER; ++e) wk[c][j][e] = w[c * DH_C + (j * 32 + lane) * R::PER + e];
        bk[c] = bias ? bias[c] : 0.f;
    }
    const int64_t row0 = (int64_t)blockIdx.x * DH_TILE;
#pragma unroll 2
    for (int i = 0; i < DH_ROWS_PER_HALF; ++i) {
        const int t = i * (DH_THREADS / 32) + half;
        const int64_t row = row0 + t;
        const int64_t rd = row < M ? row : M - 1;          // a row past the end reads the last one and is not stored
        const typename R::vec_t *src = reinterpret_cast<const typename R::vec_t *>(cat + rd * stride);
        typename R::vec_t v[R::NLOAD];
#pragma unroll
        for (int j = 0; j < R::NLOAD; ++j) v[j] = src[j * 32 + lane];
        float acc[NOUT];
#pragma unroll
        for (int c = 0; c < NOUT; ++c) acc[c] = 0.f;
#pragma unroll
        for (int j = 0; j < R::NLOAD; ++j)
#pragma unroll
            for (int e = 0; e < R::PER; ++e) {
                const float x = R::get(v[j], e);
#pragma unroll
                for (int c = 0; c < NOUT; ++c) acc[c] = fmaf(x, wk[c][j][e], acc[c]);
            }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1)
#pragma unroll
            for (int c = 0; c < NOUT; ++c) acc[c] += __shfl_xor(acc[c], o, 64);
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < NOUT; ++c) stage[c][t] = acc[c] + bk[c];
        }
    }
    __syncthreads();
    if (threadIdx.x < NOUT * DH_TILE) {
        const int c = threadIdx.x / DH_TILE, t = threadIdx.x % DH_TILE;
        const int64_t row = row0 + t;
        if (row < M) {
            const int64_t b = row / S, s = row - b * S;
            logits[(b * NOUT + c) * S + s] = stage[c][t];
        }
    }
}
static_assert(4 * DH_TILE <= DH_THREADS, "one thread per staged output");

}  // namespace

extern "C" size_t vn_rpn_iou_head_loss_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return vn_site_map_ok(B, H, W) ? VnSiteTermWs(B, H, W).bytes() : 0;
}

extern "C" int vn_rpn_iou_head_loss(const float *logits, const float *delta, const float *pos, const float *targets,
                                    const double *anchors, int32_t B, int32_t H, int32_t W, int32_t metric, void *workspace,
                                    size_t workspace_bytes, float *out2, float *d_logits, float *iou_target, vnStream stream) {
    VN_CHECK_ARG(vn_site_map_ok(B, H, W));
    VN_CHECK_ARG(metric == VN_IOU_BEV || metric == VN_IOU_3D);
    VN_CHECK_ARG(logits && delta && pos && targets && anchors && workspace && out2);
    const VnSiteTermWs ws(B, H, W);
    if (workspace_bytes < ws.bytes()) return VN_EWORKSPACE;
    hipStream_t st = vn_stream(stream);
    double *part = ws.part(workspace), *slab = ws.slab(workspace);
    const int64_t hw = (int64_t)H * W;
    k_pos_norm<VN_SITE_THREADS><<<B * VN_POS_CHUNKS, VN_SITE_THREADS, 0, st>>>(pos, hw * 2, part);
    VN_LAUNCH_STATUS();
    if (d_logits)
        k_iou_head_loss<true><<<ws.blocks, DH_THREADS, 0, st>>>(logits, delta, pos, targets, anchors, part, B, hw, metric, slab,
                                                                d_logits, iou_target);
    else
        k_iou_head_loss<false><<<ws.blocks, DH_THREADS, 0, st>>>(logits, delta, pos, targets, anchors, part, B, hw, metric, slab,
                                                                 nullptr, iou_target);
    VN_LAUNCH_STATUS();
    k_site_term_finalize<VN_SITE_THREADS><<<1, VN_SITE_THREADS, 0, st>>>(slab, ws.blocks, out2);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" int vn_iou_rectify_probs(const float *probs, const float *iou_logits, int64_t n, double alpha, float *out,
                                    vnStream stream) {
    VN_CHECK_ARG(n > 0 && n < (1ll << 31));
    VN_CHECK_ARG(std::isfinite(alpha) && alpha >= 0.0 && alpha <= 1.0);
    VN_CHECK_ARG(probs && iou_logits && out && out != probs);
    const int blocks = (int)vn_ceil_div(n, DH_THREADS);
    k_iou_rectify<<<blocks, DH_THREADS, 0, vn_stream(stream)>>>(probs, iou_logits, n, alpha, out);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" int vn_site_heads_fwd(const void *cat_rows, int32_t dtype, int64_t cat_stride, const float *w, const float *bias,
                                 int32_t n_out, int32_t B, int64_t S, float *logits, vnStream stream) {
    VN_CHECK_ARG(n_out == 2 || n_out == 4);
    VN_CHECK_ARG(dh_sizes_ok(B, S));
    VN_CHECK_ARG(dh_rows_ok(cat_rows, dtype, cat_stride));
    VN_CHECK_ARG(w && logits && reinterpret_cast<uintptr_t>(w) % 16 == 0);
    const int64_t M = (int64_t)B * S;
    const int blocks = (int)vn_ceil_div(M, DH_TILE);
    hipStream_t st = vn_stream(stream);
#define SH_FWD(DT, NOUT) k_site_heads_fwd<DT, NOUT><<<blocks, DH_THREADS, 0, st>>>(cat_rows, cat_stride, w, bias, M, S, logits)
    if (dtype == VN_BF16 && n_out == 4)
        SH_FWD(VN_BF16, 4);
    else if (dtype == VN_BF16)
        SH_FWD(VN_BF16, 2);
    else if (n_out == 4)
        SH_FWD(VN_F32, 4);
    else
        SH_FWD(VN_F32, 2);
#undef SH_FWD
    VN_LAUNCH_STATUS();
    return VN_OK;
}
