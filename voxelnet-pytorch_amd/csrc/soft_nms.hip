// Soft-NMS for the detection tail (Bodla et al., 2017): where vn_box_nms (detect.hip) DELETES every
// row that overlaps a kept row by more than a threshold, vn_box_soft_nms multiplies its score by a decreasing function of the
// overlap and walks on by the decayed scores.  Nothing is deleted (VN_SOFT_HARD excepted, which is the greedy rule restated).
//
//   k_soft_nms   one workgroup of 1024 threads per sample, a template on (method, metric).  Thread tid owns the rows
//                q * 1024 + tid, q < 4; their float64 working scores live in four register pairs, the rows' alive flags in the
//                bits of one register.  (x, y, half-diagonal) of every row sit in LDS (48 KB), as in k_dt_nms.
//                Per pick (at most post_top_k <= 64), three barriers:
//                  arg-max   every thread's best (w, row) of its alive rows; a butterfly over the 64 lanes of a wave (larger w
//                            wins, equal w goes to the smaller row: a total order, so every lane ends with the wave's best); the 16
//                            waves' results through a double-buffered LDS slot, ONE barrier (dt_next_alive's scheme); every
//                            thread reduces the 16 entries in the same order, the result is made scalar by readfirstlane: the
//                            picked row's seven fields are then scalar loads and stay out of the vector registers.
//                  near list every thread tests its alive rows: a pair whose centres are further apart than the two
//                            half-diagonals together has IoU exactly 0 under both metrics and is left alone (iou_thres >= 0, and
//                            the Gaussian factor at 0 is 1).  The others — a cluster: tens of the thousands — go into an LDS
//                            list, slots handed out by an integer atomicAdd (the list's order changes no result).
//                  clipping  entry e of the list is thread e's: box_iou_pair (common.h) on the widened rows, the IoU into LDS.
//                            Packed like this a cluster costs ONE trip through the clipping in one or two waves; left with
//                            their owners the same rows are spread over all 16 waves and four trips each (measured: 2.0-2.5x).
//                  decay     the owner reads its rows' IoUs back and applies ONE multiplication per row, so a row's product is
//                            formed in pick order: no floating-point atomics, the same bits from launch to launch.
//                The list holds one entry per thread; more near rows than that (one cluster of > 1024 rows) take further
//                trips of the same three steps.  The decay loop is `#pragma unroll 1`; the four scores ROTATE through it (slot 0
//                is the one at work, four trips bring every score home), so no register is indexed at run time.
#include "common.h"

namespace {

constexpr int SN_THREADS = 1024;
constexpr int SN_WAVES = SN_THREADS / VN_WAVE;
constexpr int SN_MAX_PRE = VN_DETECT_MAX_PRE;
constexpr int SN_MAX_POST = VN_PREDICT_MAX_TOPK;
constexpr int SN_ROWS = SN_MAX_PRE / SN_THREADS;          // rows of one thread
constexpr int SN_NONE = 0x7fffffff;

static_assert(SN_MAX_PRE % SN_THREADS == 0 && SN_ROWS >= 1 && SN_ROWS <= 4 && SN_MAX_PRE <= 65536,
              "a thread's list entries are the four 16-bit fields of one register pair; a row number fits 16 bits");
static_assert(3 * SN_MAX_PRE * sizeof(float) + 2 * SN_WAVES * (sizeof(double) + sizeof(int)) + SN_THREADS * (sizeof(double) + 2) + 4 <= 65536,
              "(x, y, half-diagonal) of every row, the arg-max slots and the near list fit the 64 KB of LDS a launch gets by default");
static_assert(SN_MAX_POST <= SN_THREADS, "one thread per output slot");

// (w, j) beats (bw, bj): the larger score, compared as numbers (-0.0 == +0.0); equal scores: the smaller row
__device__ __forceinline__ bool sn_beats(double w, int j, double bw, int bj) { return w > bw || (w == bw && j < bj); }

template <int METHOD, int METRIC>
__global__ void __launch_bounds__(SN_THREADS) k_soft_nms(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                         const int32_t *__restrict__ counts, int K, double iou_thres, double sigma,
                                                         double min_score, int post_k, int32_t *__restrict__ keep_idx,
                                                         float *__restrict__ keep_scores, int32_t *__restrict__ keep_counts) {
    __shared__ float sx[SN_MAX_PRE], sy[SN_MAX_PRE], shd[SN_MAX_PRE];
    __shared__ double best_w[2][SN_WAVES];
    __shared__ int best_j[2][SN_WAVES];
    __shared__ double near_u[SN_THREADS];          // the IoUs of one trip's near rows
    __shared__ uint16_t near_row[SN_THREADS];      // their row numbers
    __shared__ int near_cnt;
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(counts[b], 0), K);
    const float *bx = boxes + (size_t)b * K * 7;
    const float *sc = scores + (size_t)b * K;
    if (tid == 0) near_cnt = 0;
    unsigned alive = 0;          // bit q: row q * SN_THREADS + tid is eligible, not picked, not removed
    double w[SN_ROWS];
#pragma unroll
    for (int q = 0; q < SN_ROWS; ++q) w[q] = 0.0;
#pragma unroll
    for (int q = 0; q < SN_ROWS; ++q) {
        const int j = q * SN_THREADS + tid;
        if (j < n) {
            double qd[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) qd[k] = (double)bx[(size_t)j * 7 + k];
            const float s = sc[j];
            const bool ok = box_ok(qd);
            sx[j] = (float)qd[0];
            sy[j] = (float)qd[1];
            // the footprint lies within this distance of the centre; the factor covers the rounding to float32
            shd[j] = ok ? (float)(0.5 * sqrt(qd[4] * qd[4] + qd[5] * qd[5]) * 1.000001) : 0.0f;
            w[q] = (double)s;
            if (ok && isfinite(s)) alive |= 1u << q;          // an ineligible row is never kept and decays nothing
        }
    }
    __syncthreads();
    int par = 0, kept = 0;
    while (true) {
        // ---- arg-max over the alive rows
        double bw = -INFINITY;
        int bj = SN_NONE;
#pragma unroll
        for (int q = 0; q < SN_ROWS; ++q) {
            const int j = q * SN_THREADS + tid;
            if (((alive >> q) & 1u) && sn_beats(w[q], j, bw, bj)) { bw = w[q]; bj = j; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double ow = __shfl_xor(bw, o, 64);
            const int oj = __shfl_xor(bj, o, 64);
            if (sn_beats(ow, oj, bw, bj)) { bw = ow; bj = oj; }
        }
        if (lane == 0) { best_w[par][wave] = bw; best_j[par][wave] = bj; }
        __syncthreads();
        bw = best_w[par][0];
        bj = best_j[par][0];
#pragma unroll
        for (int v = 1; v < SN_WAVES; ++v) {
            const double ow = best_w[par][v];
            const int oj = best_j[par][v];
            if (sn_beats(ow, oj, bw, bj)) { bw = ow; bj = oj; }
        }
        par ^= 1;          // the next pick writes the other buffer: one barrier per pick is enough
        // every thread holds the same pair; as scalars, the picked row's fields below are scalar loads
        const int cur = __builtin_amdgcn_readfirstlane(bj);
        const uint64_t wbits = (uint64_t)__double_as_longlong(bw);
        const double wi = __longlong_as_double((long long)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(wbits >> 32)) << 32) |
                                                           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)wbits)));
        if (cur == SN_NONE || !(wi >= min_score)) break;
        if (tid == 0) {
            keep_idx[(size_t)b * post_k + kept] = cur;
            keep_scores[(size_t)b * post_k + kept] = (float)wi;
        }
        ++kept;
        if (kept == post_k) break;          // before any decay, as the greedy walk
        if ((cur & (SN_THREADS - 1)) == tid) alive &= ~(1u << (cur / SN_THREADS));          // picked
        // ---- decay: the picked row against every alive row
        double qa[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) qa[k] = (double)bx[(size_t)cur * 7 + k];
        const double xi = (double)sx[cur], yi = (double)sy[cur], hi = (double)shd[cur];
        unsigned pend = 0;          // bit q: row q is alive and near the picked row, its IoU not yet asked for
#pragma unroll
        for (int q = 0; q < SN_ROWS; ++q) {
            const int j = q * SN_THREADS + tid;
            if ((alive >> q) & 1u) {
                const double dx = (double)sx[j] - xi, dy = (double)sy[j] - yi, r = (double)shd[j] + hi;
                if (!(dx * dx + dy * dy > r * r)) pend |= 1u << q;          // else disjoint footprints: IoU exactly 0, nothing to do
            }
        }
        bool more;
        do {          // one trip unless more than SN_THREADS rows are near (near_cnt is 0 here)
            unsigned got = 0;          // bit q: row q's IoU is being computed on this trip, in entry (pos >> 16 q) & 0xffff
            uint64_t pos = 0;
#pragma unroll
            for (int q = 0; q < SN_ROWS; ++q) {
                if ((pend >> q) & 1u) {
                    const int e = atomicAdd(&near_cnt, 1);          // (an integer count: the order of the list changes no result)
                    if (e < SN_THREADS) {
                        near_row[e] = (uint16_t)(q * SN_THREADS + tid);
                        pos |= (uint64_t)e << (16 * q);
                        got |= 1u << q;
                    }
                }
            }
            pend &= ~got;
            __syncthreads();
            const int total = __builtin_amdgcn_readfirstlane(near_cnt);          // (the same word for every thread: a scalar)
            more = total > SN_THREADS;
            // the near rows, packed: entry e is thread e's, so a cluster's few dozen clippings are ONE trip of one or two waves
            if (tid < min(total, SN_THREADS)) {
                const int j = near_row[tid];
                double qb[7];
#pragma unroll
                for (int k = 0; k < 7; ++k) qb[k] = (double)bx[(size_t)j * 7 + k];
                double bev, v3;
                box_iou_pair(qa, qb, bev, v3);
                near_u[tid] = METRIC == VN_SOFT_3D ? v3 : bev;
            }
            __syncthreads();
            if (tid == 0) near_cnt = 0;          // (every thread has read it; the next atomicAdd is behind a barrier)
#pragma unroll 1
            for (int q = 0; q < SN_ROWS; ++q) {          // w[0] is row q's score on this trip
                if ((got >> q) & 1u) {
                    const double u = near_u[(int)(pos & 0xffffu)];
                    if (METHOD == VN_SOFT_HARD) {
                        if (!(u <= iou_thres)) alive &= ~(1u << q);
                    } else if (METHOD == VN_SOFT_LINEAR) {
                        if (u > iou_thres) w[0] = w[0] * (1.0 - u);
                    } else {
                        if (u > 0.0) w[0] = w[0] * exp(-(u * u) / sigma);
                    }
                }
                pos >>= 16;
                const double t = w[0];          // rotate: SN_ROWS trips bring every score home
#pragma unroll
                for (int k = 0; k + 1 < SN_ROWS; ++k) w[k] = w[k + 1];
                w[SN_ROWS - 1] = t;
            }
            if (more) __syncthreads();          // the list is filled again: behind the reset, and behind every read of near_u
        } while (more);
    }
    if (tid == 0) keep_counts[b] = kept;
    if (tid >= kept && tid < post_k) {
        keep_idx[(size_t)b * post_k + tid] = -1;
        keep_scores[(size_t)b * post_k + tid] = 0.0f;
    }
}

inline bool sn_sizes_ok(int32_t B, int32_t K, int32_t post_k) {
    return B >= 1 && K >= 1 && K <= SN_MAX_PRE && post_k >= 1 && post_k <= SN_MAX_POST;
}
inline bool sn_finite(double v) { return v - v == 0.0; }

template <int METHOD>
int sn_launch(int32_t metric, const float *boxes, const float *scores, const int32_t *counts, int32_t B, int32_t K, double iou_thres,
              double sigma, double min_score, int32_t post_k, int32_t *keep_idx, float *keep_scores, int32_t *keep_counts,
              hipStream_t st) {
    if (metric == VN_SOFT_3D)
        k_soft_nms<METHOD, VN_SOFT_3D><<<B, SN_THREADS, 0, st>>>(boxes, scores, counts, K, iou_thres, sigma, min_score, post_k, keep_idx,
                                                                 keep_scores, keep_counts);
    else
        k_soft_nms<METHOD, VN_SOFT_BEV><<<B, SN_THREADS, 0, st>>>(boxes, scores, counts, K, iou_thres, sigma, min_score, post_k, keep_idx,
                                                                  keep_scores, keep_counts);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

}  // namespace

// The kernel keeps its whole state on chip; the query answers one aligned unit for a valid size so that 0 stays the answer
// for a size the call refuses (the convention of every workspace query here).
extern "C" size_t vn_box_soft_nms_workspace_bytes(int32_t B, int32_t K) {
    if (!sn_sizes_ok(B, K, 1)) return 0;
    return vn_align(1);
}

extern "C" int vn_box_soft_nms(const float *boxes, const float *scores, const int32_t *counts, int32_t B, int32_t K, int32_t method,
                               int32_t metric, double iou_thres, double sigma, double min_score, int32_t post_top_k, int32_t *keep_idx,
                               float *keep_scores, int32_t *keep_counts, void *workspace, size_t workspace_bytes, vnStream stream) {
    VN_CHECK_ARG(boxes && scores && counts && keep_idx && keep_scores && keep_counts && workspace);
    VN_CHECK_ARG(sn_sizes_ok(B, K, post_top_k));
    VN_CHECK_ARG(method == VN_SOFT_HARD || method == VN_SOFT_LINEAR || method == VN_SOFT_GAUSSIAN);
    VN_CHECK_ARG(metric == VN_SOFT_BEV || metric == VN_SOFT_3D);
    VN_CHECK_ARG(sn_finite(iou_thres) && iou_thres >= 0.0 && iou_thres <= 1.0 && sn_finite(sigma) && sigma > 0.0 && sn_finite(min_score));
    if (workspace_bytes < vn_box_soft_nms_workspace_bytes(B, K)) return VN_EWORKSPACE;
    const hipStream_t st = vn_stream(stream);
    if (method == VN_SOFT_HARD)
        return sn_launch<VN_SOFT_HARD>(metric, boxes, scores, counts, B, K, iou_thres, sigma, min_score, post_top_k, keep_idx, keep_scores,
                                       keep_counts, st);
    if (method == VN_SOFT_LINEAR)
        return sn_launch<VN_SOFT_LINEAR>(metric, boxes, scores, counts, B, K, iou_thres, sigma, min_score, post_top_k, keep_idx, keep_scores,
                                         keep_counts, st);
    return sn_launch<VN_SOFT_GAUSSIAN>(metric, boxes, scores, counts, B, K, iou_thres, sigma, min_score, post_top_k, keep_idx, keep_scores,
                                       keep_counts, st);
}
