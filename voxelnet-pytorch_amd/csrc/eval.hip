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
//
// Image-plane scoring (KITTI's devkit rules: 2D AP, AOS, DontCare, the 2D-height bar):
//   k_boxes_to_image: one thread per detection slot: the KITTI fields of the detection under the FRAME's calibration
//            ([M | P2], 24 doubles) and the 2D box of its eight projected corners, a fully unrolled loop over registers;
//   k_eval_match_image: k_eval_match's shape with a third metric, the IoU of two axis-aligned 2D boxes.  That IoU is
//            NOT tabled: at the limits the two float64 tables already fill the 64 KB a launch gets by default, and the
//            2D IoU is eight flops, so phase 2 recomputes it from registers (the walked detection's box is shuffled
//            from the lane that owns it, the lane's two ground-truth boxes never leave it).  A detection that is off
//            the image or under the difficulty's height bar is IGNORED before the walk and takes nothing; a detection
//            the walk leaves as FP becomes IGNORED when more than half of its 2D box lies in one DontCare region.
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

// ---- image-plane scoring
constexpr int EV_MAX_DC = VN_EVAL_MAX_DC;
constexpr int EV_ROW = VN_EVAL_IMAGE_ROW;          // alpha x1 y1 x2 y2 h w l xc yc zc ry

// into (-pi, pi]
__device__ __forceinline__ double wrap_angle(double a) {
    const double pi = 3.14159265358979323846;
    return a - (2.0 * pi) * ceil((a - pi) / (2.0 * pi));
}

// IoU of two axis-aligned rectangles (x1, y1, x2, y2), areas without "+1"; 0 when the union is <= 0 (or not a number)
__device__ __forceinline__ double iou_2d(double ax1, double ay1, double ax2, double ay2, double bx1, double by1, double bx2,
                                         double by2) {
    const double iw = fmin(ax2, bx2) - fmax(ax1, bx1), ih = fmin(ay2, by2) - fmax(ay1, by1);
    const double inter = (iw > 0.0 && ih > 0.0) ? iw * ih : 0.0;
    const double uni = (ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1) - inter;
    return uni > 0.0 ? inter / uni : 0.0;
}

__global__ void __launch_bounds__(EV_THREADS) k_boxes_to_image(const float *__restrict__ det_boxes, const int32_t *__restrict__ det_counts,
                                                               const double *__restrict__ calib, const int32_t *__restrict__ image_hw,
                                                               int B, int top_k, double *__restrict__ rows,
                                                               uint8_t *__restrict__ on_image) {
    const int t = blockIdx.x * EV_THREADS + threadIdx.x;
    if (t >= B * top_k) return;
    const int b = t / top_k, d = t % top_k;
    const int nd = min(max(det_counts[b], 0), top_k);
    double o[EV_ROW];
#pragma unroll
    for (int k = 0; k < EV_ROW; ++k) o[k] = 0.0;
    bool on = false;
    double q[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) q[k] = (double)det_boxes[(size_t)t * 7 + k];
    if (d < nd && box_ok(q)) {
        double m[24];
#pragma unroll
        for (int k = 0; k < 24; ++k) m[k] = calib[(size_t)b * 24 + k];
        const double pi = 3.14159265358979323846;
        const double cx = m[0] * q[0] + m[1] * q[1] + m[2] * q[2] + m[3];
        const double cy = m[4] * q[0] + m[5] * q[1] + m[6] * q[2] + m[7];
        const double cz = m[8] * q[0] + m[9] * q[1] + m[10] * q[2] + m[11];
        const double ry = wrap_angle(-q[6] - pi / 2);
        o[0] = wrap_angle(ry - atan2(cx, cz));
        o[5] = q[3]; o[6] = q[4]; o[7] = q[5];
        o[8] = cx; o[9] = cy; o[10] = cz; o[11] = ry;
        const double cr = cos(q[6]), sr = sin(q[6]);
        const double hl = q[5] / 2, hw = q[4] / 2;
        double umin = INFINITY, umax = -INFINITY, vmin = INFINITY, vmax = -INFINITY, dmin = INFINITY;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double sx = (k & 1) ? -1.0 : 1.0, sy = (k & 2) ? -1.0 : 1.0;
            const double ax = sx * hl, ay = sy * hw;
            const double px = (ax * cr - ay * sr) + q[0];
            const double py = (ax * sr + ay * cr) + q[1];
            const double pz = (k & 4) ? q[2] + q[3] : q[2];
            const double ex = m[0] * px + m[1] * py + m[2] * pz + m[3];
            const double ey = m[4] * px + m[5] * py + m[6] * pz + m[7];
            const double ez = m[8] * px + m[9] * py + m[10] * pz + m[11];
            const double q0 = m[12] * ex + m[13] * ey + m[14] * ez + m[15];
            const double q1 = m[16] * ex + m[17] * ey + m[18] * ez + m[19];
            const double q2 = m[20] * ex + m[21] * ey + m[22] * ez + m[23];
            const double u = q0 / q2, v = q1 / q2;
            umin = fmin(umin, u); umax = fmax(umax, u);
            vmin = fmin(vmin, v); vmax = fmax(vmax, v);
            dmin = fmin(dmin, q2);
        }
        if (dmin > 0.1) {
            const double H = (double)image_hw[(size_t)b * 2], W = (double)image_hw[(size_t)b * 2 + 1];
            const double x1 = fmax(umin, 0.0), y1 = fmax(vmin, 0.0), x2 = fmin(umax, W - 1.0), y2 = fmin(vmax, H - 1.0);
            if (x2 > x1 && y2 > y1) {
                on = true;
                o[1] = x1; o[2] = y1; o[3] = x2; o[4] = y2;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < EV_ROW; ++k) rows[(size_t)t * EV_ROW + k] = o[k];
    on_image[t] = on ? 1 : 0;
}

__global__ void __launch_bounds__(EV_THREADS)
k_eval_match_image(const float *__restrict__ det_boxes, const float *__restrict__ det_scores, const int32_t *__restrict__ det_counts,
                   const double *__restrict__ gt, const int32_t *__restrict__ gt_counts, const uint8_t *__restrict__ gt_flags,
                   const double *__restrict__ rows, const uint8_t *__restrict__ on_image, const double *__restrict__ gt_bbox,
                   const double *__restrict__ gt_alpha, const double *__restrict__ dc_boxes, const int32_t *__restrict__ dc_counts,
                   const double *__restrict__ min_height, int top_k, int max_gt, int max_dc, int n_diff, double thr_bev,
                   double thr_3d, double thr_bbox, int8_t *__restrict__ status, int32_t *__restrict__ matched_gt,
                   double *__restrict__ similarity, double *__restrict__ iou_out, int32_t *__restrict__ order_out) {
    extern __shared__ double tab[];          // [2][top_k][max_gt]: BEV, 3D (the 2D IoU is recomputed in phase 2)
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nd = min(max(det_counts[b], 0), top_k);
    const int ng = min(max(gt_counts[b], 0), max_gt);
    const int ndc = max_dc > 0 ? min(max(dc_counts[b], 0), max_dc) : 0;
    const int tsz = top_k * max_gt;
    // ---- phase 1: as k_eval_match; the 2D IoU goes to iou_out only
    for (int p = tid; p < tsz; p += EV_THREADS) {
        const int d = p / max_gt, g = p % max_gt;
        double bev = 0.0, v3 = 0.0, v2 = 0.0;
        if (d < nd && g < ng) {
            double qa[7], qb[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                qa[k] = (double)det_boxes[((size_t)b * top_k + d) * 7 + k];
                qb[k] = gt[((size_t)b * max_gt + g) * 7 + k];
            }
            box_iou_pair(qa, qb, bev, v3);
            if (iou_out) {
                const double *r = rows + ((size_t)b * top_k + d) * EV_ROW;
                const double *gb = gt_bbox + ((size_t)b * max_gt + g) * 4;
                v2 = iou_2d(r[1], r[2], r[3], r[4], gb[0], gb[1], gb[2], gb[3]);
            }
        }
        tab[p] = bev;
        tab[tsz + p] = v3;
        if (iou_out) {
            iou_out[(size_t)b * 3 * tsz + p] = bev;
            iou_out[(size_t)b * 3 * tsz + tsz + p] = v3;
            iou_out[(size_t)b * 3 * tsz + 2 * (size_t)tsz + p] = v2;
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
    // ---- the lane's own detection (lane < nd): its 2D box, alpha, height, largest DontCare overlap
    double dx1 = 0.0, dy1 = 0.0, dx2 = 0.0, dy2 = 0.0, dal = 0.0, dcov = 0.0;
    bool don = false;
    if (lane < nd) {
        const double *r = rows + ((size_t)b * top_k + lane) * EV_ROW;
        dal = r[0]; dx1 = r[1]; dy1 = r[2]; dx2 = r[3]; dy2 = r[4];
        don = on_image[(size_t)b * top_k + lane] != 0;
        if (don) {
            const double area = (dx2 - dx1) * (dy2 - dy1);
            for (int j = 0; j < ndc; ++j) {
                const double *c = dc_boxes + ((size_t)b * max_dc + j) * 4;
                const double iw = fmin(dx2, c[2]) - fmax(dx1, c[0]), ih = fmin(dy2, c[3]) - fmax(dy1, c[1]);
                const double ov = (iw > 0.0 && ih > 0.0 && area > 0.0) ? (iw * ih) / area : 0.0;
                dcov = fmax(dcov, ov);
            }
        }
    }
    const double dheight = dy2 - dy1;
    // ---- the lane's two ground truths: 2D box and alpha
    const int g0 = lane, g1 = lane + 64;
    double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (g0 < ng) a0[k] = gt_bbox[((size_t)b * max_gt + g0) * 4 + k];
        if (g1 < ng) a1[k] = gt_bbox[((size_t)b * max_gt + g1) * 4 + k];
    }
    // ---- phase 2: one matching per (metric, difficulty), spread over the waves
    for (int mt = wave; mt < 3 * n_diff; mt += EV_THREADS / 64) {
        const int metric = mt / n_diff, diff = mt % n_diff;
        const double thr = metric == 0 ? thr_bev : (metric == 1 ? thr_3d : thr_bbox);
        const double *t = tab + (size_t)(metric == 1 ? 1 : 0) * tsz;
        const uint8_t *fl = gt_flags + ((size_t)b * n_diff + diff) * max_gt;
        const int c0 = g0 < ng ? (fl[g0] ? 1 : 0) : 2;          // class of the lane's two ground truths (2: not there)
        const int c1 = g1 < ng ? (fl[g1] ? 1 : 0) : 2;
        bool free0 = g0 < ng, free1 = g1 < ng;
        const double bar = min_height[diff];
        const int skip = (lane < nd && (!don || dheight < bar)) ? 1 : 0;          // off the image or under the bar
        int my_st = 0, my_mg = -1;
        for (int r = 0; r < nd; ++r) {
            const int d = __shfl(ord, r, 64);
            int bc = 2, bi = 0x7fffffff;
            double bv = 0.0;
            if (__shfl(skip, d, 64)) {          // (wave-uniform) IGNORED before the walk: takes no ground truth
                if (lane == d) { my_st = -1; my_mg = -1; }
                continue;
            }
            double v0, v1;
            if (metric == 2) {
                const double x1 = __shfl(dx1, d, 64), y1 = __shfl(dy1, d, 64), x2 = __shfl(dx2, d, 64), y2 = __shfl(dy2, d, 64);
                v0 = iou_2d(x1, y1, x2, y2, a0[0], a0[1], a0[2], a0[3]);
                v1 = iou_2d(x1, y1, x2, y2, a1[0], a1[1], a1[2], a1[3]);
            } else {
                v0 = free0 ? t[d * max_gt + g0] : 0.0;
                v1 = free1 ? t[d * max_gt + g1] : 0.0;
            }
            if (free0 && v0 > thr) { bc = c0; bv = v0; bi = g0; }
            if (free1 && v1 > thr && key_better(c1, v1, g1, bc, bv, bi)) { bc = c1; bv = v1; bi = g1; }
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
            if (lane == d) {
                my_st = bc == 0 ? 1 : (bc == 1 ? -1 : 0);
                my_mg = bc != 2 ? bi : -1;
            }
        }
        // after the walk: a false positive with more than half of its 2D box inside one DontCare region is IGNORED
        if (lane < nd && my_st == 0 && dcov > 0.5) my_st = -1;
        const size_t row = (((size_t)b * 3 + metric) * n_diff + diff) * top_k;
        if (lane < top_k) {
            status[row + lane] = lane < nd ? (int8_t)my_st : (int8_t)-2;
            matched_gt[row + lane] = lane < nd ? my_mg : -1;
            if (metric == 2) {
                double sim = 0.0;
                if (lane < nd && my_st == 1) sim = (1.0 + cos(dal - gt_alpha[(size_t)b * max_gt + my_mg])) / 2.0;
                similarity[((size_t)b * n_diff + diff) * top_k + lane] = sim;
            }
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

extern "C" int vn_boxes_to_image(const float *det_boxes, const int32_t *det_counts, const double *calib, const int32_t *image_hw,
                                 int32_t B, int32_t top_k, double *rows, uint8_t *on_image, vnStream stream) {
    VN_CHECK_ARG(B >= 0 && B <= (1 << 20) && top_k >= 1 && top_k <= EV_MAX_TOPK);
    if (B == 0) return VN_OK;
    VN_CHECK_ARG(det_boxes && det_counts && calib && image_hw && rows && on_image);
    k_boxes_to_image<<<(unsigned)vn_ceil_div((int64_t)B * top_k, EV_THREADS), EV_THREADS, 0, vn_stream(stream)>>>(
        det_boxes, det_counts, calib, image_hw, B, top_k, rows, on_image);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" int vn_eval_match_image(const float *det_boxes, const float *det_scores, const int32_t *det_counts, const double *gt,
                                   const int32_t *gt_counts, const uint8_t *gt_flags, const double *image_rows,
                                   const uint8_t *on_image, const double *gt_bbox, const double *gt_alpha, const double *dc_boxes,
                                   const int32_t *dc_counts, const double *min_height, int32_t B, int32_t top_k, int32_t max_gt,
                                   int32_t max_dc, int32_t n_diff, double thr_bev, double thr_3d, double thr_bbox, int8_t *status,
                                   int32_t *matched_gt, double *similarity, double *iou_out, void *workspace,
                                   size_t workspace_bytes, vnStream stream) {
    VN_CHECK_ARG(ev_sizes_ok(B, top_k, max_gt) && n_diff >= 1 && n_diff <= EV_MAX_DIFF && max_dc >= 0 && max_dc <= EV_MAX_DC);
    VN_CHECK_ARG(thr_bev == thr_bev && thr_3d == thr_3d && thr_bbox == thr_bbox);
    if (B == 0) return VN_OK;
    VN_CHECK_ARG(det_boxes && det_scores && det_counts && gt && gt_counts && gt_flags && status && matched_gt && workspace);
    VN_CHECK_ARG(image_rows && on_image && gt_bbox && gt_alpha && min_height && similarity);
    VN_CHECK_ARG(max_dc == 0 || (dc_boxes && dc_counts));
    VN_CHECK_ARG(workspace_bytes >= vn_eval_match_workspace_bytes(B, top_k, max_gt));
    const size_t lds = (size_t)2 * top_k * max_gt * sizeof(double);
    k_eval_match_image<<<B, EV_THREADS, lds, vn_stream(stream)>>>(
        det_boxes, det_scores, det_counts, gt, gt_counts, gt_flags, image_rows, on_image, gt_bbox, gt_alpha, dc_boxes, dc_counts,
        min_height, top_k, max_gt, max_dc, n_diff, thr_bev, thr_3d, thr_bbox, status, matched_gt, similarity, iou_out,
        static_cast<int32_t *>(workspace));
    VN_LAUNCH_STATUS();
    return VN_OK;
}
