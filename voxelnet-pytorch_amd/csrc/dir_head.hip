// Direction-classifier head of the RPN: a Conv2d(768, 2, 1) on the concatenation, one logit per anchor
// (site s, rotation a) in the site layout of prob — dir[b, a, s] —, its binary cross-entropy against the heading bin of
// the matched box, the backward of the 1x1 conv at the rows that have a gradient, and the heading-aware decode.
//   wrap_pi(x) = x - floor(x / pi) * pi                       in [0, pi)
//   bin(theta) = int(floor((theta - dir_offset) / pi)) & 1    float64
//   theta_gt   = targets[b, s, 7a + 6] + anchors[2s + a, 6]
//   bce(z, t)  = max(z, 0) - z t + log1p(exp(-|z|))
//   L_dir      = sum_b (1 / P_b) sum over positives of bce(dir[b, a, s], bin(theta_gt)),   P_b = max(1, sum pos[b])
//   decode:      r' = wrap_pi(r - dir_offset) + dir_offset + pi [dir[b, a, s] > 0]
// The 16-channel heads fill one MFMA tile (heads.hip) and stay as they are; two more outputs over 768 channels are a
// streaming dot product at 0.5 flop / byte, so the forward here uses no MFMA: half a wave per row, 16-byte loads, the
// lane's 24 x 2 weights in registers, a 5-step cross-lane reduction per output, results staged in LDS so that the two
// NCHW planes are written in runs.  The gradient is non-zero at the positive anchors only (a few dozen rows of 70,400):
// the backward compacts those rows in row order (common.h's ordered compaction) and touches nothing else.
// Sums: per-workgroup partials over the list in list order, then one fixed-order pass: no atomics, bit-identical runs.
#include <cmath>
#include "rpn_common.h"

namespace {

constexpr int DH_BWD_THREADS = 192;        // backward: 4 channels per thread
constexpr int DH_BWD_MAX_WG = 256;         // workgroups (= partial rows) of the backward's pass over the list
constexpr int DH_PART = 2 * DH_C + 2;      // one partial row: d_w[2][768], d_bias[2]
constexpr double DH_PI = 3.14159265358979323846;

// logits[b][c][s] = bias[c] + sum_k cat[b * S + s][k] * w[c][k]; products and sums fp32, the lane's 24 in channel order,
// then the butterfly over the 32 lanes.
template <int DT>
__global__ void __launch_bounds__(DH_THREADS) k_dir_head_fwd(const void *__restrict__ cat_, int64_t stride, const float *__restrict__ w,
                                                            const float *__restrict__ bias, int64_t M, int64_t S,
                                                            float *__restrict__ logits) {
    VN_PRIO_MAIN();
    typedef DhRow<DT> R;
    const typename R::elem_t *cat = static_cast<const typename R::elem_t *>(cat_);
    __shared__ float stage[2][DH_TILE];
    const int lane = threadIdx.x & 31, half = threadIdx.x >> 5;
    float w0[R::NLOAD][R::PER], w1[R::NLOAD][R::PER];
#pragma unroll
    for (int j = 0; j < R::NLOAD; ++j)
#pragma unroll
        for (int e = 0; e < R::PER; ++e) {
            const int c = (j * 32 + lane) * R::PER + e;
            w0[j][e] = w[c];
            w1[j][e] = w[DH_C + c];
        }
    const float b0 = bias ? bias[0] : 0.f, b1 = bias ? bias[1] : 0.f;
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
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int j = 0; j < R::NLOAD; ++j)
#pragma unroll
            for (int e = 0; e < R::PER; ++e) {
                const float x = R::get(v[j], e);
                a0 = fmaf(x, w0[j][e], a0);
                a1 = fmaf(x, w1[j][e], a1);
            }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            a0 += __shfl_xor(a0, o, 64);
            a1 += __shfl_xor(a1, o, 64);
        }
        if (lane == 0) {
            stage[0][t] = a0 + b0;
            stage[1][t] = a1 + b1;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * DH_TILE) {
        const int c = threadIdx.x / DH_TILE, t = threadIdx.x % DH_TILE;
        const int64_t row = row0 + t;
        if (row < M) {
            const int64_t b = row / S, s = row - b * S;
            logits[(b * 2 + c) * S + s] = stage[c][t];
        }
    }
}

// ---- backward: the rows with a gradient, in row order ----
__device__ __forceinline__ bool dh_row_listed(const float *__restrict__ d_logits, int64_t row, int64_t M, int64_t S) {
    if (row >= M) return false;
    const int64_t b = row / S, s = row - b * S;
    const float g0 = d_logits[(b * 2) * S + s], g1 = d_logits[(b * 2 + 1) * S + s];
    return g0 != 0.f || g1 != 0.f;          // (-0.0 is zero; a NaN is listed)
}

__global__ void __launch_bounds__(DH_THREADS) k_dir_bwd_count(const float *__restrict__ d_logits, int64_t M, int64_t S, int *__restrict__ cnt) {
    const int64_t row = (int64_t)blockIdx.x * DH_THREADS + threadIdx.x;
    const int n = vn_block_count(dh_row_listed(d_logits, row, M, S));
    if (threadIdx.x == 0) cnt[blockIdx.x] = n;
}

// exclusive scan of the counts in place; cnt[nb] = the total
__global__ void __launch_bounds__(DH_THREADS) k_dir_bwd_scan(int *__restrict__ cnt, int64_t nb) {
    const int total = vn_scan_block_sums<int, DH_THREADS>(cnt, nb);
    if (threadIdx.x == 0) cnt[nb] = total;
}

__global__ void __launch_bounds__(DH_THREADS) k_dir_bwd_list(const float *__restrict__ d_logits, int64_t M, int64_t S,
                                                            const int *__restrict__ cnt, int *__restrict__ list) {
    const int64_t row = (int64_t)blockIdx.x * DH_THREADS + threadIdx.x;
    const bool keep = dh_row_listed(d_logits, row, M, S);
    const int rank = vn_block_rank(keep);
    if (keep) list[cnt[blockIdx.x] + rank] = (int)row;
}

// float64 -> bf16 with ONE rounding: the fp32 in between is rounded to odd (truncated, its last bit set when inexact),
// which the nearest-even cast to bf16 then reads as the sticky bit
__device__ __forceinline__ bf16_t dh_f64_to_bf16(double x) {
    float f = (float)x;
    const double err = x - (double)f;
    if (err != 0.0 && isfinite(f) && f != 0.f) {
        uint32_t bits = __float_as_uint(f);
        if ((err > 0.0) != (f > 0.f)) bits -= 1u;          // f lies beyond x: one step back towards zero
        f = __uint_as_float(bits | 1u);
    }
    return vn_f2bf(f);
}

template <int DT> struct DhQuad;          // four consecutive channels of a row
template <> struct DhQuad<VN_BF16> {
    typedef bf16x4_t vec_t;
    static __device__ __forceinline__ float get(const vec_t &v, int e) { return vn_bf2f(v[e]); }
    static __device__ __forceinline__ void set(vec_t &v, int e, double x) { v[e] = dh_f64_to_bf16(x); }
};
template <> struct DhQuad<VN_F32> {
    typedef f32x4_t vec_t;
    static __device__ __forceinline__ float get(const vec_t &v, int e) { return v[e]; }
    static __device__ __forceinline__ void set(vec_t &v, int e, double x) { v[e] = (float)x; }
};

// workgroup g takes list entries [g * chunk, (g + 1) * chunk), chunk = ceil(n / gridDim.x), in list order; thread t owns
// channels 4t .. 4t+3.  d_cat[m] += g0 w[0] + g1 w[1] in float64 (products of two fp32 are exact there), rounded once to
// the stored type; the partial sums of g_c * cat[m] are float64 too.  A workgroup without entries writes nothing: the
// final pass reads the first ceil(n / chunk) partial rows only.
template <int DT, int DDT>
__global__ void __launch_bounds__(DH_BWD_THREADS) k_dir_bwd_rows(const float *__restrict__ d_logits, const void *__restrict__ cat_,
                                                                int64_t cat_stride, const float *__restrict__ w, int64_t S,
                                                                void *__restrict__ d_cat_, int64_t d_cat_stride,
                                                                const int *__restrict__ list, const int *__restrict__ total,
                                                                double *__restrict__ part) {
    VN_PRIO_MAIN();
    typedef DhQuad<DT> Q;
    typedef DhQuad<DDT> QD;
    const int n = *total;
    const int chunk = (n + (int)gridDim.x - 1) / (int)gridDim.x;
    const int begin = (int)blockIdx.x * chunk, end = min(n, begin + chunk);
    if (begin >= end) return;
    const int c0 = threadIdx.x * 4;
    const f32x4_t wa = *reinterpret_cast<const f32x4_t *>(w + c0), wb = *reinterpret_cast<const f32x4_t *>(w + DH_C + c0);
    double s0[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0}, sb0 = 0.0, sb1 = 0.0;
    for (int i = begin; i < end; ++i) {
        const int64_t m = list[i];
        const int64_t b = m / S, s = m - b * S;
        const double g0 = (double)d_logits[(b * 2) * S + s], g1 = (double)d_logits[(b * 2 + 1) * S + s];
        const typename Q::vec_t x = *reinterpret_cast<const typename Q::vec_t *>(
            static_cast<const char *>(cat_) + (m * cat_stride + c0) * (int64_t)(DT == VN_BF16 ? 2 : 4));
        typename QD::vec_t *dst = reinterpret_cast<typename QD::vec_t *>(
            static_cast<char *>(d_cat_) + (m * d_cat_stride + c0) * (int64_t)(DDT == VN_BF16 ? 2 : 4));
        typename QD::vec_t d = *dst;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double xe = (double)Q::get(x, e);
            s0[e] += g0 * xe;
            s1[e] += g1 * xe;
            QD::set(d, e, (double)QD::get(d, e) + g0 * (double)wa[e] + g1 * (double)wb[e]);
        }
        *dst = d;
        sb0 += g0;
        sb1 += g1;
    }
    double *p = part + (int64_t)blockIdx.x * DH_PART;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        p[c0 + e] = s0[e];
        p[DH_C + c0 + e] = s1[e];
    }
    if (threadIdx.x == 0) {
        p[2 * DH_C] = sb0;
        p[2 * DH_C + 1] = sb1;
    }
}

// one thread per output: the used partial rows in index order
__global__ void __launch_bounds__(DH_THREADS) k_dir_bwd_final(const double *__restrict__ part, const int *__restrict__ total, int nwg,
                                                             float *__restrict__ d_w, float *__restrict__ d_bias) {
    const int o = blockIdx.x * DH_THREADS + threadIdx.x;
    if (o >= DH_PART) return;
    const int n = *total;
    const int chunk = (n + nwg - 1) / nwg;
    const int used = chunk > 0 ? (n + chunk - 1) / chunk : 0;
    double s = 0.0;
#pragma unroll 8          // (the loads of eight rows in flight; the additions keep their order)
    for (int g = 0; g < used; ++g) s += part[(int64_t)g * DH_PART + o];
    if (o < 2 * DH_C)
        d_w[o] = (float)s;
    else
        d_bias[o - 2 * DH_C] = (float)s;
}

// ---- loss: rpn_common.h's site-term scaffold around k_dir_loss ----
static_assert(DH_THREADS == VN_SITE_THREADS, "k_dir_loss is launched with the scaffold's workgroup count");
__device__ __forceinline__ int dh_bin(double theta, double off) { return (int)((long long)floor((theta - off) / DH_PI) & 1ll); }

template <bool BWD>
__global__ void __launch_bounds__(DH_THREADS) k_dir_loss(const float *__restrict__ logits, const float *__restrict__ pos,
                                                        const float *__restrict__ tgt, const double *__restrict__ anchors,
                                                        const double *__restrict__ part, int B, int64_t hw, double off,
                                                        double *__restrict__ slab /* [blocks][3] */, float *__restrict__ d_logits) {
    VN_PRIO_MAIN();
    const int64_t sites = hw * B;
    const int64_t site = (int64_t)blockIdx.x * DH_THREADS + threadIdx.x;
    double s_loss = 0.0, s_hit = 0.0, s_m = 0.0;
    if (site < sites) {
        const int b = (int)(site / hw);
        const int64_t yx = site - (int64_t)b * hw;
        const float2 ps = *reinterpret_cast<const float2 *>(pos + site * 2);
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float m = a ? ps.y : ps.x;
            float out = 0.f;
            if (m != 0.f) {
                const double z = (double)logits[((int64_t)b * 2 + a) * hw + yx];
                const double theta = (double)tgt[site * 14 + a * 7 + 6] + anchors[(yx * 2 + a) * 7 + 6];
                const int t = dh_bin(theta, off);
                const double wgt = (double)m / fmax(vn_pos_total(part, b), 1.0);
                s_loss += wgt * (fmax(z, 0.0) - z * (double)t + log1p(exp(-fabs(z))));
                s_hit += ((z > 0.0) == (t == 1)) ? (double)m : 0.0;
                s_m += (double)m;
                if (BWD) out = (float)(wgt * (1.0 / (1.0 + exp(-z)) - (double)t));
            }
            if (BWD) d_logits[((int64_t)b * 2 + a) * hw + yx] = out;
        }
    }
    const double t = vn_block_sum3<DH_THREADS>(s_loss, s_hit, s_m);
    if (threadIdx.x < 3) slab[(int64_t)blockIdx.x * 3 + threadIdx.x] = t;
}

// ---- decode ----
__global__ void __launch_bounds__(DH_THREADS) k_rectify_yaw(float *__restrict__ boxes, const int32_t *__restrict__ idx,
                                                           const int32_t *__restrict__ counts, const float *__restrict__ dir_logits, int B,
                                                           int K, int n_anchors, double off) {
    const int64_t i = (int64_t)blockIdx.x * DH_THREADS + threadIdx.x;
    if (i >= (int64_t)B * K) return;
    const int b = (int)(i / K), k = (int)(i - (int64_t)b * K);
    if (k >= min(counts[b], K)) return;
    const int n = idx[i];
    if (n < 0 || n >= n_anchors) return;          // (not an anchor: the row is left as it is)
    const int64_t S = n_anchors / 2;
    const float z = dir_logits[((int64_t)b * 2 + (n & 1)) * S + (n >> 1)];
    const double x = (double)boxes[i * 7 + 6] - off;
    boxes[i * 7 + 6] = (float)((x - floor(x / DH_PI) * DH_PI) + off + (z > 0.f ? DH_PI : 0.0));
}

int dh_bwd_wgs(int64_t M) { return (int)(M < DH_BWD_MAX_WG ? M : DH_BWD_MAX_WG); }

}  // namespace

extern "C" int vn_dir_head_fwd(const void *cat_rows, int32_t dtype, int64_t cat_stride, const float *w, const float *bias, int32_t B,
                               int64_t S, float *logits, vnStream stream) {
    VN_CHECK_ARG(dh_sizes_ok(B, S));
    VN_CHECK_ARG(dh_rows_ok(cat_rows, dtype, cat_stride));
    VN_CHECK_ARG(w && logits && reinterpret_cast<uintptr_t>(w) % 16 == 0);
    const int64_t M = (int64_t)B * S;
    const int blocks = (int)vn_ceil_div(M, DH_TILE);
    hipStream_t st = vn_stream(stream);
    if (dtype == VN_BF16)
        k_dir_head_fwd<VN_BF16><<<blocks, DH_THREADS, 0, st>>>(cat_rows, cat_stride, w, bias, M, S, logits);
    else
        k_dir_head_fwd<VN_F32><<<blocks, DH_THREADS, 0, st>>>(cat_rows, cat_stride, w, bias, M, S, logits);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" size_t vn_dir_head_bwd_workspace_bytes(int32_t B, int64_t S) {
    if (!dh_sizes_ok(B, S)) return 0;
    const int64_t M = (int64_t)B * S, nb = vn_ceil_div(M, DH_THREADS);
    return vn_align(sizeof(int) * (size_t)(nb + 1)) + vn_align(sizeof(int) * (size_t)M) +
           vn_align(sizeof(double) * DH_PART * (size_t)dh_bwd_wgs(M));
}

extern "C" int vn_dir_head_bwd(const float *d_logits, const void *cat_rows, int32_t dtype, int64_t cat_stride, const float *w, int32_t B,
                               int64_t S, void *d_cat, int32_t d_cat_dtype, int64_t d_cat_stride, float *d_w, float *d_bias,
                               void *workspace, size_t workspace_bytes, vnStream stream) {
    VN_CHECK_ARG(dh_sizes_ok(B, S));
    VN_CHECK_ARG(dh_rows_ok(cat_rows, dtype, cat_stride) && dh_rows_ok(d_cat, d_cat_dtype, d_cat_stride));
    VN_CHECK_ARG(d_logits && w && d_w && d_bias && workspace && reinterpret_cast<uintptr_t>(w) % 16 == 0);
    if (workspace_bytes < vn_dir_head_bwd_workspace_bytes(B, S)) return VN_EWORKSPACE;
    const int64_t M = (int64_t)B * S, nb = vn_ceil_div(M, DH_THREADS);
    const int nwg = dh_bwd_wgs(M);
    char *p = static_cast<char *>(workspace);
    int *cnt = reinterpret_cast<int *>(p);
    p += vn_align(sizeof(int) * (size_t)(nb + 1));
    int *list = reinterpret_cast<int *>(p);
    p += vn_align(sizeof(int) * (size_t)M);
    double *part = reinterpret_cast<double *>(p);
    hipStream_t st = vn_stream(stream);
    k_dir_bwd_count<<<(int)nb, DH_THREADS, 0, st>>>(d_logits, M, S, cnt);
    VN_LAUNCH_STATUS();
    k_dir_bwd_scan<<<1, DH_THREADS, 0, st>>>(cnt, nb);
    VN_LAUNCH_STATUS();
    k_dir_bwd_list<<<(int)nb, DH_THREADS, 0, st>>>(d_logits, M, S, cnt, list);
    VN_LAUNCH_STATUS();
    const int *total = cnt + nb;
#define DH_ROWS(DT, DDT) \
    k_dir_bwd_rows<DT, DDT><<<nwg, DH_BWD_THREADS, 0, st>>>(d_logits, cat_rows, cat_stride, w, S, d_cat, d_cat_stride, list, total, part)
    if (dtype == VN_BF16 && d_cat_dtype == VN_BF16)
        DH_ROWS(VN_BF16, VN_BF16);
    else if (dtype == VN_BF16)
        DH_ROWS(VN_BF16, VN_F32);
    else if (d_cat_dtype == VN_BF16)
        DH_ROWS(VN_F32, VN_BF16);
    else
        DH_ROWS(VN_F32, VN_F32);
#undef DH_ROWS
    VN_LAUNCH_STATUS();
    k_dir_bwd_final<<<(int)vn_ceil_div(DH_PART, DH_THREADS), DH_THREADS, 0, st>>>(part, total, nwg, d_w, d_bias);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" size_t vn_rpn_dir_loss_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return vn_site_map_ok(B, H, W) ? VnSiteTermWs(B, H, W).bytes() : 0;
}

extern "C" int vn_rpn_dir_loss(const float *logits, const float *pos, const float *targets, const double *anchors, int32_t B, int32_t H,
                               int32_t W, double dir_offset, void *workspace, size_t workspace_bytes, float *out2, float *d_logits,
                               vnStream stream) {
    VN_CHECK_ARG(vn_site_map_ok(B, H, W));
    VN_CHECK_ARG(std::isfinite(dir_offset));
    VN_CHECK_ARG(logits && pos && targets && anchors && workspace && out2);
    const VnSiteTermWs ws(B, H, W);
    if (workspace_bytes < ws.bytes()) return VN_EWORKSPACE;
    hipStream_t st = vn_stream(stream);
    double *part = ws.part(workspace), *slab = ws.slab(workspace);
    const int64_t hw = (int64_t)H * W;
    k_pos_norm<VN_SITE_THREADS><<<B * VN_POS_CHUNKS, VN_SITE_THREADS, 0, st>>>(pos, hw * 2, part);
    VN_LAUNCH_STATUS();
    if (d_logits)
        k_dir_loss<true><<<ws.blocks, DH_THREADS, 0, st>>>(logits, pos, targets, anchors, part, B, hw, dir_offset, slab, d_logits);
    else
        k_dir_loss<false><<<ws.blocks, DH_THREADS, 0, st>>>(logits, pos, targets, anchors, part, B, hw, dir_offset, slab, nullptr);
    VN_LAUNCH_STATUS();
    k_site_term_finalize<VN_SITE_THREADS><<<1, VN_SITE_THREADS, 0, st>>>(slab, ws.blocks, out2);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" int vn_boxes_rectify_yaw(float *boxes, const int32_t *idx, const int32_t *counts, const float *dir_logits, int32_t B, int32_t K,
                                    int32_t n_anchors, double dir_offset, vnStream stream) {
    VN_CHECK_ARG(B > 0 && K > 0 && n_anchors > 0 && n_anchors % 2 == 0);
    VN_CHECK_ARG(std::isfinite(dir_offset));
    VN_CHECK_ARG(boxes && idx && counts && dir_logits);
    const int blocks = (int)vn_ceil_div((int64_t)B * K, DH_THREADS);
    k_rectify_yaw<<<blocks, DH_THREADS, 0, vn_stream(stream)>>>(boxes, idx, counts, dir_logits, B, K, n_anchors, dir_offset);
    VN_LAUNCH_STATUS();
    return VN_OK;
}
