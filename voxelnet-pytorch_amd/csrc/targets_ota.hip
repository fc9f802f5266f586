// RPN training targets by SimOTA (Ge et al., YOLOX, 2021) — the fourth sibling of targets.hip,
// targets_iou.hip and targets_atss.hip: same anchors, boxes and output maps, but the assignment looks at what the network
// PREDICTS.  A box takes the anchors whose decoded prediction fits it best, and how many it takes follows from how many
// predictions already overlap it.  It reads probs and deltas (site layout), so it runs after the forward.
//
// Rules (include/voxelnet_hip.h states them in full), float64 throughout.  Anchor n = site * 2 + rotation a.  For a valid box k
// (common.h box_ok) of sample b, dx = x_n - x_k, dy = y_n - y_k:
//   in_box   the anchor's centre inside the box's footprint (assign_common.h as_in_footprint: ATSS rule 5);
//   in_ctr   |dx| <= radius and |dy| <= radius;          C_k = {n : in_box or in_ctr}
//   v(n,k)   = box_iou_pair(vn_box_decode_f64(deltas of n on anchor n), gt_k), BEV or 3D
//   cost     = -log(pc) + iou_weight * -log(v + 1e-8) + (in_box and in_ctr ? 0 : 1e5),  pc = p clamped to [1e-12, 1]
//   sum_k    = the min(q, |C_k|) largest v, added in descending order;  dyn_k = max(1, floor(sum_k))
//   box k selects the dyn_k smallest (cost, n) of C_k;  matched[n] = the selecting box of the smallest cost, smallest k among
//   equals, else -1;  pos = matched >= 0;  neg = !pos.
//
// C_k has no bound (one very large box: every anchor), so it is never materialised: both selections are bounded top-q lists.
// Launches: one memset (the per-anchor words), k_ot_scan, k_ot_pick, k_as_arg, k_as_count (only with stats), k_as_encode.
//   k_ot_scan    The sites are cut into `chunks` ranges (assign_common.h as_chunks); one 64-thread workgroup per (chunk, box,
//                sample), a lane on a site and both its rotations.  The geometric test is two compares per anchor; only a
//                candidate loads its deltas and reaches the decode and the pair function.  Every lane keeps the q largest v
//                (as -v, ascending) and the q smallest (cost, n) of its candidates as sorted lists in LDS (bounded insertion,
//                the worst entry in a register); q rounds of the wave arg-min over the 64 heads rank the chunk's best q of
//                each list — exact, no barrier — which go to the workspace with the chunk's candidate count.
//   k_ot_pick    one 128-thread workgroup per (box, sample): wave 0 merges the chunks' v lists (one lane per chunk) and adds the
//                m largest in the order they come out, wave 1 merges the cost lists; then lane r < dyn_k enters its selected
//                anchor's dense word by an integer atomicMax on the complement of the cost's ordered bits (ot_key: the largest
//                complement is the smallest cost) and records (n, bits) in the workspace.
//   k_as_arg / k_as_count / k_as_encode (assign_common.h, shared with targets_atss.hip) read the RECORDED bits: nothing is
//                evaluated twice, the smallest k stays.
//   Integer atomics of an order-independent result only: outputs are bit-identical from run to run.
// LDS: k_ot_scan 64 lanes x 16 entries x (8 + 8 + 4) B = 20 KB; k_ot_pick 64 chunks x 16 x (8 + 8 + 4) B = 20 KB + 0.3 KB.
#include "assign_common.h"

namespace {

constexpr int OT_Q = VN_OTA_MAX_Q;               // entries of a list, at most; a box's recorded candidates (dyn_k <= q)
constexpr int OT_SCAN_THREADS = VN_WAVE;         // k_ot_scan: one wave, a lane per site
constexpr int OT_PICK_THREADS = 2 * VN_WAVE;     // k_ot_pick: wave 0 on the v lists, wave 1 on the cost lists
constexpr int OT_UNROLL = 4;                     // sites a lane loads before it looks at any of them
constexpr double OT_OUTSIDE = 1e5;               // the cost of a candidate that is not both in_box and in_ctr
static_assert(OT_Q <= VN_WAVE, "k_ot_pick: one lane per selected candidate");

// A double as an unsigned word of the same order (negative values too: v may round to 1, and -log(1 + 1e-8) < 0).  No cost
// is NaN, so no key is all ones and no complement is 0, the empty word.
__device__ __forceinline__ unsigned long long ot_key(double c) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(c);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ int ot_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, VN_WAVE);
    return v;
}

// part_v / part_c / part_n [B, max_gt, chunks, OT_Q]: the chunk's q largest v as -v ascending, its q smallest (cost, n)
// ascending, padded with (+inf, AS_NONE);  part_cnt [B, max_gt, chunks]: its candidates
__global__ void __launch_bounds__(OT_SCAN_THREADS) k_ot_scan(const double *__restrict__ anchors, int N, const double *__restrict__ gt,
                                                             const int32_t *__restrict__ counts, int max_gt,
                                                             const float *__restrict__ probs, const float *__restrict__ deltas,
                                                             int metric, int q, double radius, double iou_weight, int chunks,
                                                             double *__restrict__ part_v, double *__restrict__ part_c,
                                                             int32_t *__restrict__ part_n, int32_t *__restrict__ part_cnt) {
    __shared__ double l_v[OT_Q][OT_SCAN_THREADS];          // entry j of lane t at [j][t]: lanes on consecutive banks
    __shared__ double l_c[OT_Q][OT_SCAN_THREADS];
    __shared__ int32_t l_n[OT_Q][OT_SCAN_THREADS];
    const int k = blockIdx.x / chunks, ch = blockIdx.x % chunks, b = blockIdx.y, lane = threadIdx.x;
    const int G = min(max(counts[b], 0), max_gt);
    const size_t kb = (size_t)b * max_gt + k;
    double g[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) g[j] = gt[kb * 7 + j];
    if (k >= G || !box_ok(g)) return;          // (uniform over the workgroup) k_ot_pick does not read this box's lists
    const int S = N / 2;
    const int per = (S + chunks - 1) / chunks, s_lo = ch * per, s_hi = min(S, s_lo + per);
    const double cr = cos(g[6]), sr = sin(g[6]);

    // ---- scan (as_list_insert: n grows along a lane's scan; equal v need no order, they add up to the same sum)
    int cv = 0, cc = 0, cand = 0;
    double worst_v = INFINITY, worst_c = INFINITY;          // the q-th entries once the lists are full
    for (int s0 = s_lo + lane; s0 < s_hi; s0 += VN_WAVE * OT_UNROLL) {
        double x[OT_UNROLL][2], y[OT_UNROLL][2];
#pragma unroll
        for (int u = 0; u < OT_UNROLL; ++u) {
            const size_t n0 = (size_t)min(s0 + VN_WAVE * u, S - 1) * 2;
#pragma unroll
            for (int a = 0; a < 2; ++a) { x[u][a] = anchors[(n0 + a) * 7 + 0]; y[u][a] = anchors[(n0 + a) * 7 + 1]; }
        }
#pragma unroll
        for (int u = 0; u < OT_UNROLL; ++u) {
            const int s = s0 + VN_WAVE * u;
            if (s >= s_hi) continue;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const double dx = x[u][a] - g[0], dy = y[u][a] - g[1];
                const bool in_box = as_in_footprint(dx, dy, cr, sr, g);
                const bool in_ctr = fabs(dx) <= radius && fabs(dy) <= radius;          // (NaN compares false)
                if (!(in_box || in_ctr)) continue;
                ++cand;
                const int n = s * 2 + a;
                double A[7], d[7], P[7];
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    A[j] = anchors[(size_t)n * 7 + j];
                    d[j] = (double)deltas[((size_t)b * 14 + 7 * a + j) * S + s];
                }
                vn_box_decode_f64(d, A, sqrt(A[4] * A[4] + A[5] * A[5]), P);
                double vb, v3;
                box_iou_pair(P, g, vb, v3);
                double v = metric == VN_IOU_3D ? v3 : vb;
                if (!(v > 0.0)) v = 0.0;
                double pc = (double)probs[((size_t)b * 2 + a) * S + s];
                if (!(pc >= 1e-12)) pc = 1e-12;          // (a NaN p too)
                if (pc > 1.0) pc = 1.0;
                const double cost = (-log(pc) + iou_weight * (-log(v + 1e-8))) + (in_box && in_ctr ? 0.0 : OT_OUTSIDE);
                as_list_insert(l_v, lane, q, cv, worst_v, -v);
                as_list_insert(l_c, lane, q, cc, worst_c, cost, l_n, n);
            }
        }
    }

    // ---- q rounds of the wave's arg-min over the heads of its 64 sorted lists, per list; a dry round leaves the padding
    const size_t pc0 = kb * chunks + ch, po = pc0 * OT_Q;
    const int total = ot_wave_sum(cand);
    if (lane == 0) part_cnt[pc0] = total;
    int hv = 0, hc = 0;
    for (int r = 0; r < q; ++r) {
        const AsHead mv = as_merge_round(l_v, lane, lane, true, cv, hv), mc = as_merge_round(l_c, lane, lane, true, cc, hc, l_n);
        if (lane == 0) { part_v[po + r] = mv.key; part_c[po + r] = mc.key; part_n[po + r] = mc.id; }
    }
}

// stats [B, max_gt, 5] = (|C_k|, sum_k, dyn_k, the cost of the last selected candidate, [k_as_count's column])
__global__ void __launch_bounds__(OT_PICK_THREADS) k_ot_pick(int N, const double *__restrict__ gt, const int32_t *__restrict__ counts,
                                                             int max_gt, int q, int chunks, const double *__restrict__ part_v,
                                                             const double *__restrict__ part_c, const int32_t *__restrict__ part_n,
                                                             const int32_t *__restrict__ part_cnt,
                                                             unsigned long long *__restrict__ best_bits, int32_t *__restrict__ cand_n,
                                                             unsigned long long *__restrict__ cand_bits, double *__restrict__ stats) {
    __shared__ double p_v[OT_Q][AS_MAX_CHUNKS];          // entry r of chunk c at [r][c]: lanes on consecutive banks
    __shared__ double p_c[OT_Q][AS_MAX_CHUNKS];
    __shared__ int32_t p_n[OT_Q][AS_MAX_CHUNKS];
    __shared__ double s_cost[OT_Q];
    __shared__ int32_t s_n[OT_Q];
    __shared__ double s_sum;
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int G = min(max(counts[b], 0), max_gt);
    const size_t kb = (size_t)b * max_gt + k;
    double g[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) g[j] = gt[kb * 7 + j];
    const bool valid = k < G && box_ok(g);          // (uniform over the workgroup)
    const int wave = tid >> 6, lane = tid & 63;
    const int C = valid ? ot_wave_sum(lane < chunks ? part_cnt[kb * chunks + lane] : 0) : 0;
    if (C == 0) {          // no candidate, no positive, stats of zeros
        if (tid < OT_Q) { cand_n[kb * OT_Q + tid] = 0; cand_bits[kb * OT_Q + tid] = 0ull; }
        if (stats && tid < 5) stats[kb * 5 + tid] = 0.0;
        return;
    }
    const int m = min(q, C);

    // ---- merge: lane c holds chunk c's ranked list; m rounds of the wave's arg-min over the heads (the chunks hold the box's
    // m best together: every chunk kept its own q best).  Wave 0 adds the v as they come out: descending, a fixed order.
    const size_t po = (kb * chunks + min(lane, chunks - 1)) * OT_Q;
    int head = 0;
    if (wave == 0) {
        if (lane < chunks)
            for (int r = 0; r < q; ++r) p_v[r][lane] = part_v[po + r];
        double sum = 0.0;
        for (int r = 0; r < m; ++r) sum += -as_merge_round(p_v, lane, lane, lane < chunks, q, head).key;
        if (lane == 0) s_sum = sum;
    } else {
        if (lane < chunks)
            for (int r = 0; r < q; ++r) { p_c[r][lane] = part_c[po + r]; p_n[r][lane] = part_n[po + r]; }
        for (int r = 0; r < m; ++r) {
            const AsHead h = as_merge_round(p_c, lane, lane, lane < chunks, q, head, p_n);
            if (lane == 0) { s_cost[r] = h.key; s_n[r] = h.id; }
        }
    }
    __syncthreads();
    const double sum = s_sum;
    const int dyn_k = min(max(1, (int)floor(sum)), m);          // (<= m already, v <= 1: the min only bounds the reads below)
    if (tid < OT_Q) {
        unsigned long long bits = 0ull;
        int n = 0;
        if (tid < dyn_k) {
            n = s_n[tid];
            bits = ~ot_key(s_cost[tid]);
            atomicMax(best_bits + (size_t)b * N + n, bits);
        }
        cand_n[kb * OT_Q + tid] = n;
        cand_bits[kb * OT_Q + tid] = bits;
    }
    if (stats && tid == 0) {
        stats[kb * 5 + 0] = (double)C;
        stats[kb * 5 + 1] = sum;
        stats[kb * 5 + 2] = (double)dyn_k;
        stats[kb * 5 + 3] = s_cost[dyn_k - 1];
        stats[kb * 5 + 4] = 0.0;          // (k_as_count's)
    }
}

// the limits of vn_rpn_targets_atss, q in its range
inline bool ot_args_ok(int32_t B, int32_t N, int32_t max_gt, int32_t q) {
    return as_sizes_ok(B, N, max_gt) && q >= 1 && q <= VN_OTA_MAX_Q;
}

// workspace: [cost words of every anchor | ~k of every anchor | selected n | selected bits | chunk lists' -v | chunk lists' cost |
// chunk lists' n | chunk counts]; the first two are adjacent so that one memset clears both.  q does not enter: a list has
// OT_Q slots whatever it is.
struct OtaWs : AsBoxWs {
    int chunks;
    AsRegion<double> part_v, part_c;
    AsRegion<int32_t> part_n, part_cnt;
    OtaWs(int32_t B, int32_t N, int32_t max_gt) : AsBoxWs(B, N, max_gt, OT_Q), chunks(as_chunks(B, N, max_gt)) {
        part_v = add<double>((size_t)B * max_gt * chunks * OT_Q);
        part_c = add<double>((size_t)B * max_gt * chunks * OT_Q);
        part_n = add<int32_t>((size_t)B * max_gt * chunks * OT_Q);
        part_cnt = add<int32_t>((size_t)B * max_gt * chunks);
    }
};

}  // namespace

extern "C" size_t vn_rpn_targets_ota_workspace_bytes(int32_t B, int32_t n_anchors, int32_t max_gt, int32_t q) {
    if (!ot_args_ok(B, n_anchors, max_gt, q)) return 0;
    return OtaWs(B, n_anchors, max_gt).bytes();
}

extern "C" int vn_rpn_targets_ota(const double *anchors, int32_t n_anchors, const double *gt, const int32_t *gt_count, int32_t B,
                                  int32_t max_gt, const float *probs, const float *deltas, int32_t metric, int32_t q, double radius,
                                  double iou_weight, double anchor_h, float *pos, float *neg, float *targets, int32_t *matched,
                                  double *stats, void *workspace, size_t workspace_bytes, vnStream stream) {
    VN_CHECK_ARG(anchors && gt && gt_count && probs && deltas && pos && neg && targets && workspace &&
                 ot_args_ok(B, n_anchors, max_gt, q) && anchor_h != 0.0);
    VN_CHECK_ARG(metric == VN_IOU_BEV || metric == VN_IOU_3D);
    VN_CHECK_ARG(radius >= 0.0 && std::isfinite(radius) && iou_weight >= 0.0 && std::isfinite(iou_weight));          // (NaN: false)
    const OtaWs ws(B, n_anchors, max_gt);
    if (workspace_bytes < ws.bytes()) return VN_EWORKSPACE;
    hipStream_t st = vn_stream(stream);
    const int chunks = ws.chunks;
    unsigned long long *best_bits = ws.best_bits(workspace), *cand_bits = ws.cand_bits(workspace);
    int32_t *cand_n = ws.cand_n(workspace), *part_n = ws.part_n(workspace), *part_cnt = ws.part_cnt(workspace);
    double *part_v = ws.part_v(workspace), *part_c = ws.part_c(workspace);
    VN_HIP(hipMemsetAsync(best_bits, 0, ws.dense_bytes, st));
    const dim3 boxes((unsigned)max_gt, (unsigned)B);
    k_ot_scan<<<dim3((unsigned)(max_gt * chunks), (unsigned)B), OT_SCAN_THREADS, 0, st>>>(
        anchors, n_anchors, gt, gt_count, max_gt, probs, deltas, metric, q, radius, iou_weight, chunks, part_v, part_c, part_n, part_cnt);
    VN_LAUNCH_STATUS();
    k_ot_pick<<<boxes, OT_PICK_THREADS, 0, st>>>(n_anchors, gt, gt_count, max_gt, q, chunks, part_v, part_c, part_n, part_cnt, best_bits,
                                                 cand_n, cand_bits, stats);
    VN_LAUNCH_STATUS();
    return as_launch_tail<OT_Q>(ws, workspace, st, anchors, n_anchors, gt, B, max_gt, anchor_h, pos, neg, targets, matched, stats, 5, 4);
}
