// Detection scoring on the device — the stage the reference leaves empty (voxelnet/eval.py:4-5 is a stub; protocol:
// DESIGN.md section 1b): the IoU of two ROTATED boxes in the bird's-eye view and in 3D, and the per-frame greedy
// matching of vn_rpn_predict's detections against the frame's ground truths that a KITTI-style average precision
// needs.  The host (voxelnet_amd/evaluate.py) only accumulates one status byte per detection and does the O(detections)
// precision / recall arithmetic.
//
// Box = (x, y, z, h, w, l, r) in the lidar frame (targets.py): footprint corners (+-l/2, +-w/2) turned by r about
// (x, y), vertical extent [z, z + h].  All arithmetic is float64 (a float32 detection is widened exactly), written
// as in tests/eval_ref.py, no contraction (-ffp-contract=off).
//
// BEV intersection: both footprints are translated so that A's centre is the origin (no cancellation of 70-m
// coordinates in the shoelace sum); A's rectangle is clipped by the four half-planes of B (Sutherland-Hodgman) and the
// polygon's area is the shoelace sum.  The polygon has at most 8 vertices.  It lives in REGISTERS: every read is at a
// compile-time index of a fully unrolled loop, and "append at position n" is a select over the 8 slots — a
// runtime-indexed private array would be placed in scratch memory by this compiler.  A vertex appended to a full
// polygon is dropped (it cannot happen for convex input in exact arithmetic), so nothing is ever indexed out of range.
//
//   iou_bev = I / (wa*la + wb*lb - I)
//   iou_3d  = I*zo / (ha*wa*la + hb*wb*lb - I*zo),  zo = max(0, min(za+ha, zb+hb) - max(za, zb))
// A pair scores 0, never NaN, when a field is not finite, when w, l or h of either box is <= 0, or when the
// denominator is <= 0.
//
// Matching (one workgroup of 4 wave64 per frame):
//   phase 1: all 256 threads fill the frame's BEV and 3D IoU tables in LDS, one clipping per pair
//            (2 x top_k x max_gt doubles: 2 x 20 KB at 20 x 128, 64 KB at the limits 32 x 128);
//   phase 2: the 2 * n_diff matchings (metric x difficulty) are spread over the four waves.  A wave walks the
//            detections by descending score (ties: lower index); its lanes own the ground truths (lane, lane + 64);
//            the detection's choice among the free ground truths with IoU > thr is a wave arg-max on the key
//            (valid before ignored, IoU descending, index ascending) — a total order, so the result does not depend
//            on the lane order of the reduction.
// No host synchronisation: the detection counts are read on the device.
// The pair function (box_iou_pair and its helpers) lives in common.h: detect.hip's rotated NMS calls it too.
#include "common.h"

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_MAX_TOPK = VN_EVAL_MAX_TOPK;
constexpr int EV_MAX_GT = VN_TARGETS_MAX_GT;
constexpr int EV_MAX_DIFF = VN_EVAL_MAX_DIFF;

static_assert(EV_MAX_TOPK <= VN_WAVE, "a lane per detection when the wave ranks the scores");
static_assert(EV_MAX_GT <= 2 * VN_WAVE, "two ground truths per lane");
static_assert(2 * EV_MAX_TOPK * EV_MAX_GT * sizeof(double) <= 65536, "both IoU tables fit the 64 KB of LDS a launch gets by default");

__global__ void __launch_bounds__(EV_THREADS) k_box_iou_rotated(const double *__restrict__ a, int na, const double *__restrict__ b,
                                                                int nb, int metric, double *__restrict__ out) {
    const int64_t p = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x;
    if (p >= (int64_t)na * nb) return;
    const int i = (int)(p / nb), j = (int)(p % nb);
    double qa[7], qb[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { qa[k] = a[(size_t)i * 7 + k]; qb[k] = b[(size_t)j * 7 + k]; }
    double bev, v3;
    box_iou_pair(qa, qb, bev, v3);
    out[p] = metric == 0 ? bev : v3;
}

// the matcher's key: class 0 = a valid ground truth, 1 = an ignored one, 2 = nothing to take
__device__ __forceinline__ bool key_better(int c1, double v1, int i1, int c2, double v2, int i2) {
    return c1 < c2 || (c1 == c2 && (v1 > v2 || (v1 == v2 && i1 < i2)));
}

__global__ void __launch_bounds__(EV_THREADS) k_eval_match(const float *__restrict__ det_boxes, const float *__restrict__ det_scores,
                                                           const int32_t *__restrict__ det_counts, const double *__restrict__ gt,
                                                           const int32_t *__restrict__ gt_counts, const uint8_t *__restrict__ gt_flags,
                                                           int top_k, int max_gt, int n_diff, double thr_bev, double thr_3d,
                                                           int8_t *__restrict__ status, int32_t *__restrict__ matched_gt,
                                                           double *__restrict__ iou_out, int32_t *__restrict__ order_out) {
    extern __shared__ double tab[];          // [2][top_k][max_gt]
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nd = min(max(det_counts[b], 0), top_k);
    const int ng = min(max(gt_counts[b], 0), max_gt);
    const int tsz = top_k * max_gt;
    // ---- phase 1: the two IoU tables of the frame (slots beyond the counts: 0)
    for (int p = tid; p < tsz; p += EV_THREADS) {
        const int d = p / max_gt, g = p % max_gt;
        double bev = 0.0, v3 = 0.0;
        if (d < nd && g < ng) {
            double qa[7], qb[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                qa[k] = (double)det_boxes[((size_t)b * top_k + d) * 7 + k];
                qb[k] = gt[((size_t)b * max_gt + g) * 7 + k];
            }
            box_iou_pair(qa, qb, bev, v3);
        }
        tab[p] = bev;
        tab[tsz + p] = v3;
        if (iou_out) {
            iou_out[(size_t)b * 2 * tsz + p] = bev;
            iou_out[(size_t)b * 2 * tsz + tsz + p] = v3;
        }
    }
    __syncthreads();
    // ---- the walk order: lane r ends up with the detection of rank r (score descending, ties by lower index)
    float sc = -INFINITY;
    if (lane < nd) {
        sc = det_scores[(size_t)b * top_k + lane];
        if (!(sc == sc)) sc = -INFINITY;          // a NaN score ranks last
    }
    int rank = 0;
    for (int j = 0; j < nd; ++j) {
        const float sj = __shfl(sc, j, 64);
        rank += (sj > sc || (sj == sc && j < lane)) ? 1 : 0;
    }
    int ord = 0;
    for (int j = 0; j < nd; ++j) {
        const int rj = __shfl(rank, j, 64);
        if (rj == lane) ord = j;
    }
    if (wave == 0 && lane < top_k) order_out[(size_t)b * top_k + lane] = lane < nd ? ord : -1;
    // ---- phase 2: one matching per (metric, difficulty), spread over the waves
    for (int mt = wave; mt < 2 * n_diff; mt += EV_THREADS / 64) {
        const int metric = mt / n_diff, diff = mt % n_diff;
        const double thr = metric == 0 ? thr_bev : thr_3d;
        const double *t = tab + (size_t)metric * tsz;
        const uint8_t *fl = gt_flags + ((size_t)b * n_diff + diff) * max_gt;
        const int g0 = lane, g1 = lane + 64;
        const int c0 = g0 < ng ? (fl[g0] ? 1 : 0) : 2;          // class of the lane's two ground truths (2: not there)
        const int c1 = g1 < ng ? (fl[g1] ? 1 : 0) : 2;
        bool free0 = g0 < ng, free1 = g1 < ng;
        int8_t *st = status + (((size_t)b * 2 + metric) * n_diff + diff) * top_k;
        int32_t *mg = matched_gt + (((size_t)b * 2 + metric) * n_diff + diff) * top_k;
        for (int r = 0; r < nd; ++r) {
            const int d = __shfl(ord, r, 64);
            int bc = 2, bi = 0x7fffffff;
            double bv = 0.0;
            if (free0) {
                const double v = t[d * max_gt + g0];
                if (v > thr) { bc = c0; bv = v; bi = g0; }
            }
            if (free1) {
                const double v = t[d * max_gt + g1];
                if (v > thr && key_better(c1, v, g1, bc, bv, bi)) { bc = c1; bv = v; bi = g1; }
            }
            for (int o = 32; o > 0; o >>= 1) {
                const int oc = __shfl_xor(bc, o, 64);
                const double ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (key_better(oc, ov, oi, bc, bv, bi)) { bc = oc; bv = ov; bi = oi; }
            }
            if (bc != 2) {          // a taken ground truth, valid or ignored, is gone for the later detections
                if (bi == g0) free0 = false;
                if (bi == g1) free1 = false;
            }
            if (lane == 0) {
                st[d] = bc == 0 ? (int8_t)1 : (bc == 1 ? (int8_t)-1 : (int8_t)0);
                mg[d] = bc != 2 ? bi : -1;
            }
        }
        for (int d = nd + lane; d < top_k; d += 64) {
            st[d] = (int8_t)-2;
            mg[d] = -1;
        }
    }
}

inline bool ev_sizes_ok(int32_t B, int32_t top_k, int32_t max_gt) {
    return B >= 0 && B <= (1 << 20) && top_k >= 1 && top_k <= EV_MAX_TOPK && max_gt >= 1 && max_gt <= EV_MAX_GT;
}

}  // namespace

extern "C" int vn_box_iou_rotated(const double *a, int32_t na, const double *b, int32_t nb, int32_t metric, double *out,
                                  vnStream stream) {
    VN_CHECK_ARG(na >= 0 && nb >= 0 && (metric == VN_EVAL_BEV || metric == VN_EVAL_3D));
    VN_CHECK_ARG((int64_t)na * nb < (1ll << 31));
    if (na == 0 || nb == 0) return VN_OK;
    VN_CHECK_ARG(a && b && out);
    const int64_t pairs = (int64_t)na * nb;
    k_box_iou_rotated<<<(unsigned)vn_ceil_div(pairs, EV_THREADS), EV_THREADS, 0, vn_stream(stream)>>>(a, na, b, nb, metric, out);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" size_t vn_eval_match_workspace_bytes(int32_t B, int32_t top_k, int32_t max_gt) {
    if (!ev_sizes_ok(B, top_k, max_gt) || B == 0) return 0;
    return vn_align((size_t)B * top_k * sizeof(int32_t));          // the walk order of every frame
}

extern "C" int vn_eval_match(const float *det_boxes, const float *det_scores, const int32_t *det_counts, const double *gt,
                             const int32_t *gt_counts, const uint8_t *gt_flags, int32_t B, int32_t top_k, int32_t max_gt,
                             int32_t n_diff, double thr_bev, double thr_3d, int8_t *status, int32_t *matched_gt, double *iou_out,
                             void *workspace, size_t workspace_bytes, vnStream stream) {
    VN_CHECK_ARG(ev_sizes_ok(B, top_k, max_gt) && n_diff >= 1 && n_diff <= EV_MAX_DIFF);
    VN_CHECK_ARG(thr_bev == thr_bev && thr_3d == thr_3d);
    if (B == 0) return VN_OK;
    VN_CHECK_ARG(det_boxes && det_scores && det_counts && gt && gt_counts && gt_flags && status && matched_gt && workspace);
    VN_CHECK_ARG(workspace_bytes >= vn_eval_match_workspace_bytes(B, top_k, max_gt));
    const size_t lds = (size_t)2 * top_k * max_gt * sizeof(double);
    k_eval_match<<<B, EV_THREADS, lds, vn_stream(stream)>>>(det_boxes, det_scores, det_counts, gt, gt_counts, gt_flags, top_k, max_gt,
                                                           n_diff, thr_bev, thr_3d, status, matched_gt, iou_out,
                                                           static_cast<int32_t *>(workspace));
    VN_LAUNCH_STATUS();
    return VN_OK;
}
