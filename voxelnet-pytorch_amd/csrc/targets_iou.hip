// RPN training targets by a REAL IoU — beside targets.hip, which keeps the reference's assignment
// with its zero-extent anchor rectangles and its (y1 - x1 + 1) union term.  Same inputs minus the host-made gt_standup,
// same three output maps, plus the matched ground-truth index of every anchor.
//
// Rules (include/voxelnet_hip.h states them in full).  IoU(n,k) in float64, one of
//   VN_ASSIGN_STANDUP  the axis-aligned hulls x +- (l|cos r| + w|sin r|)/2, y +- (l|sin r| + w|cos r|)/2 of the two rotated
//                      footprints, areas without "+1", 0 when the hulls do not overlap (overlap written from the centres);
//   VN_ASSIGN_ROTATED  common.h box_iou_pair's iou_bev of (anchor, box): 0 for a box that fails box_ok.
// m_n = max_k IoU(n,k) at its smallest k = k_n;  M_k = max_n IoU(n,k) at its smallest n = n_k.
// matched[n] = k_n when m_n >= pos_iou, else the smallest k with n_k == n and M_k > 0, else -1;  pos = matched >= 0;
// neg = m_n < neg_iou and not pos (every anchor of a sample without a box).
//
// Launches: one memset (per-box maxima and arg-max words), k_ti_pairs twice, k_ti_encode.
//   k_ti_pairs phase 0  one thread per anchor, the sample's boxes in LDS: every IoU once, m_n / k_n to the workspace, and
//                       M_k by an integer atomicMax on the IoU's float64 bits (a non-negative double orders as its bits).
//              phase 1  THE SAME CODE OBJECT again (phase is an argument: the IoUs come out bit for bit as in phase 0):
//                       an anchor whose IoU with box k equals M_k enters n_k by an atomicMax on ~n.  Only boxes with
//                       0 < M_k < pos_iou are visited: with M_k >= pos_iou the anchor n_k is positive through m_n already.
//   Integer atomics of an order-independent result: deterministic from run to run; no floating-point atomics.
//   Rotated kind: a pair whose centres are further apart than the two half-diagonals together has disjoint footprints, the
//   pair function returns exactly 0 for it, and it is skipped without clipping (k_dt_nms's reject): ~1,000 of the 70,400
//   anchors reach the float64 clipping per box.
//   k_ti_encode         matched, pos, neg and the seven regression targets (rpn_common.h's vn_box_encode, as k_tg_encode) of every anchor.
#include "assign_common.h"

namespace {

constexpr int TI_THREADS = 256;
constexpr int TI_MAX_GT = VN_TARGETS_MAX_GT;

// (ti_pair_side / ti_pair_iou: assign_common.h, shared with targets_atss.hip)

template <int KIND>
__global__ void __launch_bounds__(TI_THREADS) k_ti_pairs(const double *__restrict__ anchors, int N, const double *__restrict__ gt,
                                                         const int32_t *__restrict__ counts, int max_gt, int phase, double pos_iou,
                                                         double *__restrict__ best_iou, int32_t *__restrict__ best_k,
                                                         unsigned long long *__restrict__ box_max, uint32_t *__restrict__ box_arg) {
    __shared__ double sg[TI_MAX_GT][7];          // the boxes
    __shared__ double sd[TI_MAX_GT][5];          // stand-up: ti_hull's five; rotated: [0] = half-diagonal, < 0 for an invalid box
    __shared__ unsigned long long smax[TI_MAX_GT];          // phase 1: M_k's bits, 0 for a box that is not visited
    const int b = blockIdx.y, G = min(max(counts[b], 0), max_gt);
    for (int k = threadIdx.x; k < G; k += TI_THREADS) {
        double q[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) { q[j] = gt[((size_t)b * max_gt + k) * 7 + j]; sg[k][j] = q[j]; }
        double h[5];
        ti_pair_side<KIND>(q, h);
#pragma unroll
        for (int j = 0; j < ti_side_len<KIND>(); ++j) sd[k][j] = h[j];
        unsigned long long mk = 0;
        if (phase == 1) {
            mk = box_max[(size_t)b * max_gt + k];
            if (!(__longlong_as_double((long long)mk) < pos_iou)) mk = 0;          // n_k is positive through m_n already
        }
        smax[k] = mk;
    }
    __syncthreads();
    const int n = blockIdx.x * TI_THREADS + threadIdx.x;
    if (n >= N) return;
    double a[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) a[j] = anchors[(size_t)n * 7 + j];
    double ah[5];
    ti_pair_side<KIND>(a, ah);
    double m = 0.0;
    int kn = 0;
#pragma unroll 1
    for (int k = 0; k < G; ++k) {
        if (phase == 1 && smax[k] == 0) continue;
        double v = 0.0;
        if (!ti_pair_iou<KIND>(a, ah, sg[k], sd[k], v)) continue;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
        if (phase == 0) {
            if (v > m) { m = v; kn = k; }          // strict: the smallest k of the maximum
            atomicMax(box_max + (size_t)b * max_gt + k, bits);
        } else if (bits == smax[k]) {
            atomicMax(box_arg + (size_t)b * max_gt + k, ~(uint32_t)n);          // the smallest n of the maximum
        }
    }
    if (phase == 0) {
        best_iou[(size_t)b * N + n] = m;
        best_k[(size_t)b * N + n] = kn;
    }
}

__global__ void __launch_bounds__(TI_THREADS) k_ti_encode(const double *__restrict__ anchors, int N, const double *__restrict__ gt,
                                                          const int32_t *__restrict__ counts, int max_gt,
                                                          const double *__restrict__ best_iou, const int32_t *__restrict__ best_k,
                                                          const unsigned long long *__restrict__ box_max,
                                                          const uint32_t *__restrict__ box_arg, double pos_iou, double neg_iou,
                                                          double anchor_h, float *__restrict__ pos, float *__restrict__ neg,
                                                          float *__restrict__ targets, int32_t *__restrict__ matched) {
    __shared__ int garg[TI_MAX_GT];          // n_k of the boxes with 0 < M_k < pos_iou, else -1
    const int b = blockIdx.y, G = min(max(counts[b], 0), max_gt);
    for (int k = threadIdx.x; k < G; k += TI_THREADS) {
        const double mk = __longlong_as_double((long long)box_max[(size_t)b * max_gt + k]);
        garg[k] = (mk > 0.0 && mk < pos_iou) ? (int)~box_arg[(size_t)b * max_gt + k] : -1;
    }
    __syncthreads();
    const int n = blockIdx.x * TI_THREADS + threadIdx.x;
    if (n >= N) return;
    const size_t o = (size_t)b * N + n;
    const double m = best_iou[o];
    int box = -1;
    if (G > 0) {
        if (m >= pos_iou) {
            box = best_k[o];
        } else {
            for (int k = 0; k < G; ++k)
                if (garg[k] == n) { box = k; break; }
        }
    }
    as_write_targets(o, box, box < 0 && (G == 0 || m < neg_iou), gt + (size_t)b * max_gt * 7, anchors + (size_t)n * 7, anchor_h, pos, neg,
                     targets, matched);
}

// workspace: [m_n | k_n | M_k bits | ~n_k]; the last two are adjacent so that one memset clears both
struct TiWs : AsLayout {
    AsRegion<double> best_iou;
    AsRegion<int32_t> best_k;
    AsRegion<unsigned long long> box_max;
    AsRegion<uint32_t> box_arg;
    TiWs(int32_t B, int32_t N, int32_t max_gt) {
        best_iou = add<double>((size_t)B * N);
        best_k = add<int32_t>((size_t)B * N);
        box_max = add<unsigned long long>((size_t)B * max_gt);
        box_arg = add<uint32_t>((size_t)B * max_gt);
    }
    size_t box_bytes() const { return total - box_max.off; }          // the memset
};

template <int KIND>
int ti_launch_pairs(dim3 grid, hipStream_t st, const double *anchors, int N, const double *gt, const int32_t *counts, int max_gt,
                    double pos_iou, double *best_iou, int32_t *best_k, unsigned long long *box_max, uint32_t *box_arg) {
    for (int phase = 0; phase < 2; ++phase) {
        k_ti_pairs<KIND><<<grid, TI_THREADS, 0, st>>>(anchors, N, gt, counts, max_gt, phase, pos_iou, best_iou, best_k, box_max, box_arg);
        VN_LAUNCH_STATUS();
    }
    return VN_OK;
}

}  // namespace

extern "C" size_t vn_rpn_targets_iou_workspace_bytes(int32_t B, int32_t n_anchors, int32_t max_gt) {
    if (!tg_sizes_ok(B, n_anchors, max_gt)) return 0;
    return TiWs(B, n_anchors, max_gt).bytes();
}

extern "C" int vn_rpn_targets_iou(const double *anchors, int32_t n_anchors, const double *gt, const int32_t *gt_count, int32_t B,
                                  int32_t max_gt, int32_t iou_kind, float pos_iou, float neg_iou, double anchor_h, float *pos,
                                  float *neg, float *targets, int32_t *matched, void *workspace, size_t workspace_bytes,
                                  vnStream stream) {
    VN_CHECK_ARG(anchors && gt && gt_count && pos && neg && targets && workspace && tg_sizes_ok(B, n_anchors, max_gt) &&
                 anchor_h != 0.0);
    VN_CHECK_ARG(iou_kind == VN_ASSIGN_STANDUP || iou_kind == VN_ASSIGN_ROTATED);
    VN_CHECK_ARG(pos_iou == pos_iou && neg_iou == neg_iou);          // a NaN threshold
    const TiWs ws(B, n_anchors, max_gt);
    if (workspace_bytes < ws.bytes()) return VN_EWORKSPACE;
    hipStream_t st = vn_stream(stream);
    double *best_iou = ws.best_iou(workspace);
    int32_t *best_k = ws.best_k(workspace);
    unsigned long long *box_max = ws.box_max(workspace);
    uint32_t *box_arg = ws.box_arg(workspace);
    VN_HIP(hipMemsetAsync(box_max, 0, ws.box_bytes(), st));
    const dim3 grid((unsigned)((n_anchors + TI_THREADS - 1) / TI_THREADS), (unsigned)B);
    const double pd = (double)pos_iou, nd = (double)neg_iou;
    const int rc = iou_kind == VN_ASSIGN_STANDUP
                       ? ti_launch_pairs<VN_ASSIGN_STANDUP>(grid, st, anchors, n_anchors, gt, gt_count, max_gt, pd, best_iou, best_k,
                                                            box_max, box_arg)
                       : ti_launch_pairs<VN_ASSIGN_ROTATED>(grid, st, anchors, n_anchors, gt, gt_count, max_gt, pd, best_iou, best_k,
                                                            box_max, box_arg);
    if (rc != VN_OK) return rc;
    k_ti_encode<<<grid, TI_THREADS, 0, st>>>(anchors, n_anchors, gt, gt_count, max_gt, best_iou, best_k, box_max, box_arg, pd, nd,
                                            anchor_h, pos, neg, targets, matched);
    VN_LAUNCH_STATUS();
    return VN_OK;
}
