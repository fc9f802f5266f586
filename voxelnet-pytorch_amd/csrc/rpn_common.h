// Shared by the RPN tail — iou_loss.hip, dir_head.hip, iou_head.hip, predict.hip, detect.hip and, through assign_common.h, the
// four targets*.hip — and by nothing else: the ONE copy of the anchor box codec, of the rows of the concatenation as the 1x1
// heads read them, and of the scaffold of a loss term summed over the (B, h, w) anchor sites.  What only the
// target assigners share is in assign_common.h.  common.h goes into every translation unit; the two kernels here do not
// belong in the convolution files.
#pragma once
#include "common.h"

namespace {

// ---- anchor box codec: box (x, y, z, h, w, l, r), anchor a likewise, diag = sqrt(a.w^2 + a.l^2) ----
// Two decodes, on purpose.  vn_box_decode_f32 is the reference's inference tail bit for bit (deltas_to_boxes_3d,
// utils.py:476-489): float64 arithmetic on fp32 deltas, a float32 exp, the class's anchor_h for z, float32 boxes.
// vn_box_decode_f64 is the differentiable form of the IoU loss: float64 throughout, a double exp, the
// anchor's own height for z; the caller passes diag because the chain rule through the decode needs it again.
__device__ __forceinline__ void vn_box_decode_f32(const float (&d)[7], const double *a, double anchor_h, float (&o)[7]) {
    const double diag = sqrt(a[4] * a[4] + a[5] * a[5]);
    o[0] = (float)((double)d[0] * diag + a[0]);
    o[1] = (float)((double)d[1] * diag + a[1]);
    o[2] = (float)((double)d[2] * anchor_h + a[2]);
    o[3] = (float)((double)expf(d[3]) * a[3]);
    o[4] = (float)((double)expf(d[4]) * a[4]);
    o[5] = (float)((double)expf(d[5]) * a[5]);
    o[6] = (float)((double)d[6] + a[6]);
}

__device__ __forceinline__ void vn_box_decode_f64(const double (&d)[7], const double (&A)[7], double diag, double (&P)[7]) {
    P[0] = d[0] * diag + A[0];
    P[1] = d[1] * diag + A[1];
    P[2] = d[2] * A[3] + A[2];
    P[3] = exp(d[3]) * A[3];
    P[4] = exp(d[4]) * A[4];
    P[5] = exp(d[5]) * A[5];
    P[6] = d[6] + A[6];
}

// The IoU VALUE of the pair an anchor's regression channels dp and its targets dg decode to: what
// iou_loss.hip differentiates and iou_head.hip takes as the confidence head's target.  -> false for an invalid pair — a
// decoded field not finite, a size not > 0, the area (bev) / volume (3d) sum not finite —, which scores 0 (ib = i3 = 0).
// P, G, diag, S = the areas' sum and V = the volumes' sum are what the derivative needs again.
__device__ __forceinline__ bool vn_iou_pair_value(const double (&dp)[7], const double (&dg)[7], const double (&A)[7], int metric,
                                                  double &diag, double (&P)[7], double (&G)[7], double &S, double &V, double &ib,
                                                  double &i3) {
    ib = 0.0;
    i3 = 0.0;
    S = 0.0;
    V = 0.0;
    diag = sqrt(A[4] * A[4] + A[5] * A[5]);
    vn_box_decode_f64(dp, A, diag, P);
    vn_box_decode_f64(dg, A, diag, G);
    if (!(box_ok(P) && box_ok(G))) return false;
    const double area_p = P[4] * P[5], area_g = G[4] * G[5];
    S = area_p + area_g;
    V = P[3] * area_p + G[3] * area_g;
    if (!isfinite(metric == VN_IOU_3D ? V : S)) return false;
    box_iou_pair(P, G, ib, i3);
    return true;
}

// the regression targets of ground-truth box g on anchor a (utils.py:390-392): float64 arithmetic, float32 storage
__device__ __forceinline__ void vn_box_encode(const double *g, const double *a, double anchor_h, float (&t)[7]) {
    const double diag = sqrt(a[4] * a[4] + a[5] * a[5]);
    t[0] = (float)((g[0] - a[0]) / diag);
    t[1] = (float)((g[1] - a[1]) / diag);
    t[2] = (float)((g[2] - a[2]) / anchor_h);
    t[3] = (float)log(g[3] / a[3]);
    t[4] = (float)log(g[4] / a[4]);
    t[5] = (float)log(g[5] / a[5]);
    t[6] = (float)(g[6] - a[6]);
}

// stand-up rectangle (x1, y1, x2, y2) of a float32 box (utils.py:230-252, 283-330): float64 rotation, float32 corners
__device__ __forceinline__ void vn_box_standup_f32(const float (&o)[7], float (&r)[4]) {
    const double x = o[0], y = o[1], w = o[4], l = o[5], yaw = o[6];
    const double c = cos(yaw), s = sin(yaw);
    const double fx[4] = {-l / 2, -l / 2, l / 2, l / 2}, fy[4] = {w / 2, -w / 2, -w / 2, w / 2};
    float x1 = INFINITY, y1 = INFINITY, x2 = -INFINITY, y2 = -INFINITY;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float cx = (float)((c * fx[q] + (-s) * fy[q]) + x);      // np.dot row, then + translation; float32 store
        const float cy = (float)((s * fx[q] + c * fy[q]) + y);
        x1 = fminf(x1, cx); x2 = fmaxf(x2, cx);
        y1 = fminf(y1, cy); y2 = fmaxf(y2, cy);
    }
    r[0] = x1; r[1] = y1; r[2] = x2; r[3] = y2;
}

// ---- rows of the concatenation, as the 1x1 heads on it read them (dir_head.hip, iou_head.hip) ----
constexpr int DH_C = 768;                  // channels of the concatenation
constexpr int DH_THREADS = 256;
constexpr int DH_TILE = 64;                // rows per workgroup of a head's forward: 8 half-waves x 8 rows
constexpr int DH_ROWS_PER_HALF = DH_TILE / (DH_THREADS / 32);

// The 24 channels of lane l (of 32) of a row, as NLOAD 16-byte loads of PER channels each: channel (j * 32 + l) * PER + e.
template <int DT> struct DhRow;
template <> struct DhRow<VN_BF16> {
    static constexpr int NLOAD = 3, PER = 8;
    typedef bf16x8_t vec_t;
    typedef bf16_t elem_t;
    static __device__ __forceinline__ float get(const vec_t &v, int e) { return vn_bf2f(v[e]); }
};
template <> struct DhRow<VN_F32> {
    static constexpr int NLOAD = 6, PER = 4;
    typedef f32x4_t vec_t;
    typedef float elem_t;
    static __device__ __forceinline__ float get(const vec_t &v, int e) { return v[e]; }
};

bool dh_sizes_ok(int32_t B, int64_t S) { return B > 0 && S > 0 && (int64_t)B * S < (1ll << 31); }
bool dh_rows_ok(const void *p, int32_t dtype, int64_t stride) {
    if (dtype != VN_BF16 && dtype != VN_F32) return false;          // (the split [hi|lo] formats are not handled here)
    const int64_t per16 = dtype == VN_BF16 ? 8 : 4;
    return p && stride >= DH_C && stride % per16 == 0 && reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

// ---- site-term scaffold: loss = sum_b (1 / P_b) sum over positives of a per-anchor term, P_b = max(1, sum pos[b]) ----
// Three launches, all sums float64 in a fixed order (no atomics, bit-identical runs): k_pos_norm, 16 workgroups per sample,
// leaves partial sums of pos; the term's own kernel (k_iou_loss, k_dir_loss, k_iou_head_loss), one thread per site, adds a sample's
// partials with vn_pos_total and writes one slab row of three sums per workgroup; k_site_term_finalize adds the rows.
constexpr int VN_SITE_THREADS = 256;
constexpr int VN_POS_CHUNKS = 16;          // workgroups per sample in k_pos_norm

// the sum of three doubles per thread over a THREADS-thread workgroup, fixed order; thread k < 3 returns sum k
template <int THREADS>
__device__ __forceinline__ double vn_block_sum3(double s0, double s1, double s2) {
    __shared__ double red[3][THREADS / 64];
    double v[3] = {s0, s1, s2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < 3)
        for (int w = 0; w < THREADS / 64; ++w) t += red[threadIdx.x][w];
    return t;
}

// The two kernels are templates on the workgroup size (always VN_SITE_THREADS) so that only the files that launch them
// instantiate them: a plain __global__ function would be compiled into the code object of every includer.
// part[b * VN_POS_CHUNKS + chunk] = partial sum of pos[b] (per_b elements per sample)
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_pos_norm(const float *__restrict__ pos, int64_t per_b, double *__restrict__ part) {
    VN_PRIO_MAIN();
    const int b = blockIdx.x / VN_POS_CHUNKS, chunk = blockIdx.x % VN_POS_CHUNKS;
    double s = 0.0;
    for (int64_t i = (int64_t)chunk * THREADS + threadIdx.x; i < per_b; i += (int64_t)VN_POS_CHUNKS * THREADS)
        s += (double)pos[(int64_t)b * per_b + i];
    const double t = vn_block_sum3<THREADS>(s, 0.0, 0.0);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// sum pos[b]: the sample's partials in index order
__device__ __forceinline__ double vn_pos_total(const double *__restrict__ part, int b) {
    double pb = 0.0;
    for (int c = 0; c < VN_POS_CHUNKS; ++c) pb += part[(int64_t)b * VN_POS_CHUNKS + c];
    return pb;
}

// slab [nblocks][3] -> out2[0] = sum0, out2[1] = sum1 / max(sum2, 1); one workgroup, the rows in a fixed order
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_site_term_finalize(const double *__restrict__ slab, int nblocks, float *__restrict__ out2) {
    VN_PRIO_MAIN();
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblocks; i += THREADS)
        for (int k = 0; k < 3; ++k) s[k] += slab[(int64_t)i * 3 + k];
    const double t = vn_block_sum3<THREADS>(s[0], s[1], s[2]);
    __shared__ double tot[3];
    if (threadIdx.x < 3) tot[threadIdx.x] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        out2[0] = (float)tot[0];
        out2[1] = (float)(tot[1] / fmax(tot[2], 1.0));
    }
}

bool vn_site_map_ok(int32_t B, int32_t H, int32_t W) { return B > 0 && H > 0 && W > 0 && (int64_t)B * H * W < (1ll << 31); }

// workspace of a site term: [k_pos_norm's partials | the slab]; `blocks` = workgroups of the term's kernel = slab rows
struct VnSiteTermWs {
    int blocks;
    size_t part_bytes, slab_bytes;
    VnSiteTermWs(int32_t B, int32_t H, int32_t W)
        : blocks((int)vn_ceil_div((int64_t)B * H * W, VN_SITE_THREADS)),
          part_bytes(vn_align(sizeof(double) * VN_POS_CHUNKS * (size_t)B)),
          slab_bytes(vn_align(sizeof(double) * 3 * (size_t)blocks)) {}
    size_t bytes() const { return part_bytes + slab_bytes; }
    double *part(void *ws) const { return static_cast<double *>(ws); }
    double *slab(void *ws) const { return reinterpret_cast<double *>(static_cast<char *>(ws) + part_bytes); }
};

}  // namespace
