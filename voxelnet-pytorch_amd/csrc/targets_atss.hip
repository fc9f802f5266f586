// RPN training targets by ATSS (Zhang et al., CVPR 2020) — the third sibling of targets.hip and
// targets_iou.hip: same anchors, boxes and output maps, but every ground-truth box sets ITS OWN IoU threshold from the
// anchors nearest to it, and there are no pos_iou / neg_iou.
//
// Rules (include/voxelnet_hip.h states them in full), float64 throughout.  Anchor n = site * 2 + rotation; group a = the
// anchors with (n & 1) == a.  For a valid box k (common.h box_ok) of sample b:
//   d2(n,k) = dx*dx + dy*dy, dx = x_n - x_k, dy = y_n - y_k;
//   C_k     = per group the min(top_k, n_anchors / 2) anchors with the smallest (d2, n), lexicographic;
//   v(n,k)  = the IoU vn_rpn_targets_iou computes for the pair (assign_common.h ti_pair_iou: ti_standup_iou / common.h box_iou_pair);
//   mu, sd  = mean and unbiased standard deviation of v over C_k, summed in candidate order (group 0 by rank, then
//             group 1 by rank);  t = mu + sd;
//   accepted: v >= t, v > 0, and the anchor's centre inside the box's footprint (|u| <= l/2 along the box's length axis,
//             |w'| <= w/2 along its width axis, edges inside);
//   matched[n] = the accepting box of the largest v, the smallest k among equals, else -1;  pos = matched >= 0;  neg = !pos.
//
// Launches: one memset (the per-anchor words), k_as_scan, k_as_pick, k_as_arg, k_as_count (only with stats), k_as_encode.
//   k_as_scan    The sites are cut into `chunks` equal ranges (as_chunks: enough workgroups to fill the device when there
//                are few boxes, at least 64 sites each); one 128-thread workgroup per (chunk, box, sample), wave a on
//                group a.  Every lane keeps the top_k best (d2, n) of the sites it visits as a sorted list in LDS (bounded
//                insertion; its worst entry stays in registers, so an anchor that does not enter costs one compare); then
//                top_k rounds of a wave-wide arg-min over the 64 list heads rank the chunk's best top_k — exact, no
//                barrier inside the merge — which go to the workspace, padded with (+inf, INT_MAX).
//   k_as_pick    one 128-thread workgroup per (box, sample): wave a merges its group's `chunks` ranked lists the same way
//                (one lane per chunk), one lane per candidate evaluates v, thread 0 adds the <= 64 values in candidate
//                order, and an accepted candidate enters the dense per-anchor word by an integer atomicMax on v's float64
//                bits (a non-negative double orders as its bits) and is recorded, bits and all, in the workspace.
//   (k_as_arg, k_as_count, k_as_encode, the lists, the wave arg-min and the footprint test: assign_common.h, shared with targets_ota.hip)
//   k_as_arg     reads the RECORDED bits (nothing is evaluated twice): where they equal the anchor's maximum, an atomicMax
//                on ~k leaves the smallest k.
//   k_as_count   stats[..., 3]: a box counts its own recorded candidates that it won — no atomics.
//   k_as_encode  matched, pos, neg and the seven regression targets of every anchor, as k_ti_encode.
//   Integer atomics of an order-independent result only: outputs are bit-identical from run to run.
// LDS: k_as_scan 128 lanes x 32 entries x (8 + 4) B = 48 KB of lists, k_as_pick 2 x 64 chunks x 32 x (8 + 4) B = 48 KB + 1.3 KB:
// one workgroup's static allocation, three workgroups fit the CU's 160 KB.  Only the 2 * top_k candidates of a box reach the
// pair function.
#include "assign_common.h"

namespace {

constexpr int AS_THREADS = 128;                  // k_as_scan, k_as_pick: two waves, one per rotation group
constexpr int AS_K = VN_ATSS_MAX_TOPK;
constexpr int AS_CAND = 2 * AS_K;                // candidates of a box, at most: one wave
constexpr int AS_UNROLL = 8;                     // sites a lane loads before it looks at any of them
static_assert(AS_CAND == VN_WAVE, "one lane per candidate");

// part_d / part_n [B, max_gt, chunks, 2, AS_K]: the K best (d2, n) of group a inside chunk c, ascending
__global__ void __launch_bounds__(AS_THREADS) k_as_scan(const double *__restrict__ anchors, int N, const double *__restrict__ gt,
                                                        const int32_t *__restrict__ counts, int max_gt, int top_k, int chunks,
                                                        double *__restrict__ part_d, int32_t *__restrict__ part_n) {
    __shared__ double l_d[AS_K][AS_THREADS];          // entry j of lane t at [j][t]: lanes on consecutive banks
    __shared__ int32_t l_n[AS_K][AS_THREADS];
    const int k = blockIdx.x / chunks, ch = blockIdx.x % chunks, b = blockIdx.y, tid = threadIdx.x;
    const int G = min(max(counts[b], 0), max_gt);
    const size_t kb = (size_t)b * max_gt + k;
    double q[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = gt[kb * 7 + j];
    if (k >= G || !box_ok(q)) return;          // (uniform over the workgroup) k_as_pick does not read this box's lists
    const int S = N / 2, K = min(top_k, S);          // sites; candidates per group
    const int a = tid >> 6, lane = tid & 63;
    const int per = (S + chunks - 1) / chunks, s_lo = ch * per, s_hi = min(S, s_lo + per);

    // ---- scan: this lane's K best (d2, n) of group a, ascending (as_list_insert: n grows along the scan)
    int c = 0;
    double worst = INFINITY;          // the K-th entry once the list is full
    for (int s0 = s_lo + lane; s0 < s_hi; s0 += VN_WAVE * AS_UNROLL) {
        double x[AS_UNROLL], y[AS_UNROLL];
#pragma unroll
        for (int u = 0; u < AS_UNROLL; ++u) {
            const int s = s0 + VN_WAVE * u;
            const size_t n = (size_t)min(s, S - 1) * 2 + a;
            x[u] = anchors[n * 7 + 0];
            y[u] = anchors[n * 7 + 1];
        }
#pragma unroll
        for (int u = 0; u < AS_UNROLL; ++u) {
            const int s = s0 + VN_WAVE * u;
            const double dx = x[u] - q[0], dy = y[u] - q[1];
            double d = dx * dx + dy * dy;
            if (!(d == d)) d = INFINITY;          // an anchor without a position ranks last
            if (s < s_hi) as_list_insert(l_d, tid, K, c, worst, d, l_n, s * 2 + a);
        }
    }

    // ---- K rounds of the wave's arg-min over the heads of its 64 sorted lists; a chunk of fewer than K sites runs dry
    const size_t po = ((kb * chunks + ch) * 2 + a) * AS_K;
    int head = 0;
    for (int r = 0; r < K; ++r) {
        const AsHead m = as_merge_round(l_d, tid, lane, true, c, head, l_n);
        if (lane == 0) { part_d[po + r] = m.key; part_n[po + r] = m.id; }
    }
}

template <int KIND>
__global__ void __launch_bounds__(AS_THREADS) k_as_pick(const double *__restrict__ anchors, int N, const double *__restrict__ gt,
                                                        const int32_t *__restrict__ counts, int max_gt, int top_k, int chunks,
                                                        const double *__restrict__ part_d, const int32_t *__restrict__ part_n,
                                                        unsigned long long *__restrict__ best_bits, int32_t *__restrict__ cand_n,
                                                        unsigned long long *__restrict__ cand_bits, double *__restrict__ stats) {
    __shared__ double p_d[2][AS_K][AS_MAX_CHUNKS];          // entry r of chunk c at [a][r][c]: lanes on consecutive banks
    __shared__ int32_t p_n[2][AS_K][AS_MAX_CHUNKS];
    __shared__ int32_t s_cand[2][AS_K];
    __shared__ double s_v[AS_CAND];
    __shared__ double s_stat[3];
    const int k = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int G = min(max(counts[b], 0), max_gt);
    const size_t kb = (size_t)b * max_gt + k;
    double q[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = gt[kb * 7 + j];
    if (k >= G || !box_ok(q)) {          // (uniform over the workgroup) no candidates, no positive, stats of zeros
        if (tid < AS_CAND) { cand_n[kb * AS_CAND + tid] = 0; cand_bits[kb * AS_CAND + tid] = 0ull; }
        if (stats && tid < 4) stats[kb * 4 + tid] = 0.0;
        return;
    }
    const int S = N / 2, K = min(top_k, S);
    const int a = tid >> 6, lane = tid & 63;

    // ---- merge: lane c of wave a holds chunk c's ranked list of group a; K rounds of the wave's arg-min over the heads
    // (the chunks hold the group's K best together: every chunk kept its own K best)
    if (lane < chunks) {
        const size_t po = ((kb * chunks + lane) * 2 + a) * AS_K;
        for (int r = 0; r < K; ++r) { p_d[a][r][lane] = part_d[po + r]; p_n[a][r][lane] = part_n[po + r]; }
    }
    int head = 0;
    for (int r = 0; r < K; ++r) {
        const AsHead m = as_merge_round(p_d[a], lane, lane, lane < chunks, K, head, p_n[a]);
        if (lane == 0) s_cand[a][r] = m.id;
    }
    __syncthreads();

    // ---- one lane per candidate: v(n,k) exactly as k_ti_pairs evaluates the pair
    const int C = 2 * K;
    int n = 0;
    double an[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, v = 0.0;
    if (tid < C) {
        n = s_cand[tid / K][tid % K];
#pragma unroll
        for (int j = 0; j < 7; ++j) an[j] = anchors[(size_t)n * 7 + j];
        double ah[5], gh[5];
        ti_pair_side<KIND>(an, ah);
        ti_pair_side<KIND>(q, gh);
        if (!ti_pair_iou<KIND>(an, ah, q, gh, v)) v = 0.0;
        s_v[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {          // the <= 64 values in candidate order: a fixed order of additions
        double sum = 0.0;
        for (int i = 0; i < C; ++i) sum += s_v[i];
        const double mu = sum / (double)C;
        double ss = 0.0;
        for (int i = 0; i < C; ++i) { const double e = s_v[i] - mu; ss += e * e; }
        const double sd = sqrt(ss / (double)(C - 1));
        s_stat[0] = mu; s_stat[1] = sd; s_stat[2] = mu + sd;
        if (stats) { stats[kb * 4 + 0] = mu; stats[kb * 4 + 1] = sd; stats[kb * 4 + 2] = mu + sd; }
    }
    __syncthreads();
    if (tid < AS_CAND) {
        unsigned long long bits = 0ull;
        if (tid < C && v > 0.0 && v >= s_stat[2]) {
            if (as_in_footprint(an[0] - q[0], an[1] - q[1], cos(q[6]), sin(q[6]), q)) bits = (unsigned long long)__double_as_longlong(v);
        }
        if (bits) atomicMax(best_bits + (size_t)b * N + n, bits);
        cand_n[kb * AS_CAND + tid] = n;
        cand_bits[kb * AS_CAND + tid] = bits;
    }
}

// the limits of vn_rpn_targets_iou, an even anchor count, top_k in its range
inline bool as_args_ok(int32_t B, int32_t N, int32_t max_gt, int32_t top_k) {
    return as_sizes_ok(B, N, max_gt) && top_k >= 1 && top_k <= VN_ATSS_MAX_TOPK;
}

// workspace: [v bits of every anchor | ~k of every anchor | candidates' n | candidates' bits | chunk lists' d2 | chunk lists' n];
// the first two are adjacent so that one memset clears both.  top_k does not enter: a box records AS_CAND slots whatever it is.
struct AtssWs : AsBoxWs {
    int chunks;
    AsRegion<double> part_d;
    AsRegion<int32_t> part_n;
    AtssWs(int32_t B, int32_t N, int32_t max_gt) : AsBoxWs(B, N, max_gt, AS_CAND), chunks(as_chunks(B, N, max_gt)) {
        part_d = add<double>((size_t)B * max_gt * chunks * AS_CAND);
        part_n = add<int32_t>((size_t)B * max_gt * chunks * AS_CAND);
    }
};

}  // namespace

extern "C" size_t vn_rpn_targets_atss_workspace_bytes(int32_t B, int32_t n_anchors, int32_t max_gt, int32_t top_k) {
    if (!as_args_ok(B, n_anchors, max_gt, top_k)) return 0;
    return AtssWs(B, n_anchors, max_gt).bytes();
}

extern "C" int vn_rpn_targets_atss(const double *anchors, int32_t n_anchors, const double *gt, const int32_t *gt_count, int32_t B,
                                   int32_t max_gt, int32_t iou_kind, int32_t top_k, double anchor_h, float *pos, float *neg,
                                   float *targets, int32_t *matched, double *stats, void *workspace, size_t workspace_bytes,
                                   vnStream stream) {
    VN_CHECK_ARG(anchors && gt && gt_count && pos && neg && targets && workspace && as_args_ok(B, n_anchors, max_gt, top_k) &&
                 anchor_h != 0.0);
    VN_CHECK_ARG(iou_kind == VN_ASSIGN_STANDUP || iou_kind == VN_ASSIGN_ROTATED);
    const AtssWs ws(B, n_anchors, max_gt);
    if (workspace_bytes < ws.bytes()) return VN_EWORKSPACE;
    hipStream_t st = vn_stream(stream);
    const int chunks = ws.chunks;
    unsigned long long *best_bits = ws.best_bits(workspace), *cand_bits = ws.cand_bits(workspace);
    int32_t *cand_n = ws.cand_n(workspace), *part_n = ws.part_n(workspace);
    double *part_d = ws.part_d(workspace);
    VN_HIP(hipMemsetAsync(best_bits, 0, ws.dense_bytes, st));
    const dim3 boxes((unsigned)max_gt, (unsigned)B);
    k_as_scan<<<dim3((unsigned)(max_gt * chunks), (unsigned)B), AS_THREADS, 0, st>>>(anchors, n_anchors, gt, gt_count, max_gt, top_k,
                                                                                     chunks, part_d, part_n);
    VN_LAUNCH_STATUS();
    if (iou_kind == VN_ASSIGN_STANDUP)
        k_as_pick<VN_ASSIGN_STANDUP><<<boxes, AS_THREADS, 0, st>>>(anchors, n_anchors, gt, gt_count, max_gt, top_k, chunks, part_d, part_n,
                                                                   best_bits, cand_n, cand_bits, stats);
    else
        k_as_pick<VN_ASSIGN_ROTATED><<<boxes, AS_THREADS, 0, st>>>(anchors, n_anchors, gt, gt_count, max_gt, top_k, chunks, part_d, part_n,
                                                                   best_bits, cand_n, cand_bits, stats);
    VN_LAUNCH_STATUS();
    return as_launch_tail<AS_CAND>(ws, workspace, st, anchors, n_anchors, gt, B, max_gt, anchor_h, pos, neg, targets, matched, stats, 4, 3);
}
