// Test-time augmentation and box voting for the detection tail, beside detect.hip: what an
// evaluation script does AFTER the greedy NMS of section 1c has picked one box per cluster.
//
//   k_tta_merge       vn_pool_merge.  One workgroup per sample: the candidate pools of V views (vn_rpn_select_decode's
//                     output per view) become ONE priority order.  64-bit keys — k_dt_filter's order-preserving score bits
//                     in the high word, ~src in the low word (src = v * K + k: equal scores put the smaller src first) —
//                     sorted in LDS by k_dt_select's descending bitonic network (<= 4096 x 8 B = 32 KB); then one thread
//                     per output row gathers the row and maps it back to the frame's own coordinates: the exact inverse of
//                     stages 2-4 of augment.compose_affine (flip, rotation, scaling; views carry no translation), float64
//                     on the widened fields, one float32 store.  The view table travels as a kernel argument.  No atomics.
//   k_tta_vote        vn_box_vote.  One workgroup of 256 per (kept entry, sample): the kept row of vn_box_nms is replaced by
//                     the weighted mean of its cluster — every row whose BEV IoU (common.h box_iou_pair) with it is >=
//                     vote_thres.  Each thread strides over the rows with eight float64 partial sums, V float maxima (the
//                     best member score per view) and a member count; a pair whose centres are further apart than the two
//                     half-diagonals together is skipped without clipping (k_dt_nms' test: exact, vote_thres > 0).  Wave
//                     butterflies over 64 lanes, then the four waves through LDS in wave order: no floating-point atomics,
//                     two launches give the same bits.
//   k_tta_vote_order  one wave per sample: the <= 64 voted rows by descending output score (ties: walk order), skipped
//                     entries closed up.
#include "common.h"

namespace {

constexpr int TT_MERGE_THREADS = 1024;
constexpr int TT_VOTE_THREADS = 256;
constexpr int TT_VOTE_WAVES = TT_VOTE_THREADS / VN_WAVE;
constexpr int TT_MAX_ROWS = VN_DETECT_MAX_PRE;
constexpr int TT_MAX_KEEP = VN_PREDICT_MAX_TOPK;
constexpr int TT_MAX_VIEWS = VN_TTA_MAX_VIEWS;
constexpr double TT_PI = 3.14159265358979323846;

static_assert((TT_MAX_ROWS & (TT_MAX_ROWS - 1)) == 0, "the bitonic network sorts a power of two");
static_assert(TT_MAX_ROWS * sizeof(uint64_t) + 64 <= 65536, "the keys fit the 64 KB of LDS a launch gets by default");
static_assert(TT_MAX_KEEP <= VN_WAVE, "one lane per kept entry in the ordering pass");

// the views as the merge kernel takes them (a kernel argument): c, s = cos / sin of the angle, computed once on the host
struct TtViews {
    double fy[TT_MAX_VIEWS], c[TT_MAX_VIEWS], s[TT_MAX_VIEWS], angle[TT_MAX_VIEWS], factor[TT_MAX_VIEWS];
    int32_t identity[TT_MAX_VIEWS];          // fy = +1, angle = 0, factor = 1: the row is copied bit for bit
};

// k_dt_filter's map (detect.hip dt_key): the unsigned order of the result is the order of the scores; -0.0 == +0.0
__device__ __forceinline__ uint32_t tt_score_bits(float p) {
    const uint32_t u = p == 0.0f ? 0u : __float_as_uint(p);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(TT_MERGE_THREADS) k_tta_merge(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                                const int32_t *__restrict__ counts, const TtViews views, int V, int B,
                                                                int K, float *__restrict__ out_boxes, float *__restrict__ out_scores,
                                                                int32_t *__restrict__ out_src, int32_t *__restrict__ out_counts) {
    __shared__ uint64_t skey[TT_MAX_ROWS];
    __shared__ int s_n;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int rows = V * K;          // <= TT_MAX_ROWS (checked on the host)
    int P = 1;
    while (P < rows) P <<= 1;
    if (tid == 0) s_n = 0;
    // a key per row of every view; 0 (below every key: a score's high word is > 0) for a row past its view's count, a NaN
    // score and the padding up to the power of two
    for (int c = tid; c < P; c += TT_MERGE_THREADS) {
        uint64_t key = 0;
        if (c < rows) {
            const int v = c / K, k = c - v * K;
            const int cnt = min(max(counts[v * B + b], 0), K);
            if (k < cnt) {
                const float p = scores[((size_t)v * B + b) * K + k];
                if (p == p) key = ((uint64_t)tt_score_bits(p) << 32) | (uint32_t)~(uint32_t)c;
            }
        }
        skey[c] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += TT_MERGE_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const uint64_t a = skey[i], c = skey[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? a < c : a > c) { skey[i] = c; skey[l] = a; }
                }
            }
            __syncthreads();
        }
    }
    // the number of rows: the position behind the last key that is not 0 (exactly one thread sees it)
    for (int c = tid; c < P; c += TT_MERGE_THREADS)
        if (skey[c] != 0 && (c + 1 == P || skey[c + 1] == 0)) s_n = c + 1;
    __syncthreads();
    const int n = s_n;
    if (tid == 0) out_counts[b] = n;
    for (int t = tid; t < n; t += TT_MERGE_THREADS) {
        const int src = (int)~(uint32_t)(skey[t] & 0xffffffffull);
        const int v = src / K, k = src - v * K;
        const size_t in = ((size_t)v * B + b) * K + k, out = (size_t)b * rows + t;
        float o[7];
#pragma unroll
        for (int f = 0; f < 7; ++f) o[f] = boxes[in * 7 + f];
        // the view's fields by fixed index (a dynamic index into a kernel argument would go through scratch)
        double fy = 1.0, cs = 1.0, sn = 0.0, ang = 0.0, fac = 1.0;
        bool ident = true;
#pragma unroll
        for (int u = 0; u < TT_MAX_VIEWS; ++u) {
            if (u == v) {
                fy = views.fy[u]; cs = views.c[u]; sn = views.s[u]; ang = views.angle[u]; fac = views.factor[u];
                ident = views.identity[u] != 0;
            }
        }
        if (!ident) {
            double q[6];
#pragma unroll
            for (int f = 0; f < 6; ++f) q[f] = (double)o[f] / fac;
            const double X = q[0] * cs - q[1] * sn, Y = q[0] * sn + q[1] * cs;
            const double r = (double)o[6] + ang;
            o[0] = (float)X;
            o[1] = (float)(fy * Y);
#pragma unroll
            for (int f = 2; f < 6; ++f) o[f] = (float)q[f];
            o[6] = (float)(fy * r);
        }
#pragma unroll
        for (int f = 0; f < 7; ++f) out_boxes[out * 7 + f] = o[f];
        out_scores[out] = scores[in];
        out_src[out] = src;
    }
}

__device__ __forceinline__ double tt_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void tt_load_row(const float *__restrict__ bx, int j, double (&q)[7]) {
#pragma unroll
    for (int k = 0; k < 7; ++k) q[k] = (double)bx[(size_t)j * 7 + k];
}

// the voted rows of one (kept entry, sample) into the workspace: [B,P,7] fields | [B,P] score | [B,P] members | [B,P] valid
__global__ void __launch_bounds__(TT_VOTE_THREADS) k_tta_vote(const float *__restrict__ boxes, const float *__restrict__ scores,
                                                              const int32_t *__restrict__ counts, const int32_t *__restrict__ src,
                                                              int rows_per_view, const int32_t *__restrict__ keep_idx,
                                                              const int32_t *__restrict__ keep_counts, int K, int P, int V,
                                                              double vote_thres, int weight_mode, int score_mode,
                                                              float *__restrict__ w_boxes, float *__restrict__ w_scores,
                                                              int32_t *__restrict__ w_members, int32_t *__restrict__ w_valid) {
    __shared__ double s_sum[TT_VOTE_WAVES][8];
    __shared__ float s_max[TT_VOTE_WAVES][TT_MAX_VIEWS];
    __shared__ int s_cnt[TT_VOTE_WAVES];
    const int t = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(counts[b], 0), K);
    const int m = min(max(keep_counts[b], 0), P);
    if (t >= m) return;          // workgroup-uniform
    const size_t slot = (size_t)b * P + t;
    const int i = keep_idx[slot];
    const float *bx = boxes + (size_t)b * K * 7;
    const float *sc = scores + (size_t)b * K;
    const int32_t *sv = src ? src + (size_t)b * K : nullptr;
    double qi[7];
    bool ok_i = i >= 0 && i < n;
    if (ok_i) {
        tt_load_row(bx, i, qi);
        ok_i = box_ok(qi);
    }
    if (!ok_i) {          // never produced by vn_box_nms: the entry is skipped (workgroup-uniform)
        if (tid == 0) w_valid[slot] = 0;
        return;
    }
    const double hd_i = 0.5 * sqrt(qi[4] * qi[4] + qi[5] * qi[5]) * 1.000001;
    double sum[8];          // sum w | sum w q0..q5 | sum w d
#pragma unroll
    for (int k = 0; k < 8; ++k) sum[k] = 0.0;
    float best[TT_MAX_VIEWS];
#pragma unroll
    for (int v = 0; v < TT_MAX_VIEWS; ++v) best[v] = -INFINITY;
    int members = 0;
#pragma unroll 1
    for (int j = tid; j < n; j += TT_VOTE_THREADS) {
        double qj[7];
        tt_load_row(bx, j, qj);
        double u = 1.0;
        if (j != i) {
            if (!box_ok(qj)) continue;
            const double dx = qj[0] - qi[0], dy = qj[1] - qi[1];
            const double r = 0.5 * sqrt(qj[4] * qj[4] + qj[5] * qj[5]) * 1.000001 + hd_i;
            if (dx * dx + dy * dy > r * r) continue;          // disjoint footprints: IoU exactly 0 < vote_thres
            double v3;
            box_iou_pair(qi, qj, u, v3);
            if (!(u >= vote_thres)) continue;
        }
        const float sf = sc[j];
        const double s = (double)sf;
        const double w = weight_mode == VN_VOTE_W_SCORE_IOU ? s * u : s;
        const double dr = qj[6] - qi[6];
        const double d = dr - TT_PI * floor(dr / TT_PI + 0.5);          // a member that points the other way: the same axis
        sum[0] += w;
#pragma unroll
        for (int k = 0; k < 6; ++k) sum[1 + k] += w * qj[k];
        sum[7] += w * d;
        ++members;
        int view = 0;
        if (sv) {
            const int sj = sv[j];
            view = sj >= 0 ? sj / rows_per_view : -1;
        }
#pragma unroll
        for (int v = 0; v < TT_MAX_VIEWS; ++v) best[v] = (v == view) ? fmaxf(best[v], sf) : best[v];
    }
    // 64 lanes by butterflies (every lane ends with the wave's value), then the four waves in wave order
#pragma unroll
    for (int k = 0; k < 8; ++k) sum[k] = tt_wave_sum(sum[k]);
#pragma unroll
    for (int v = 0; v < TT_MAX_VIEWS; ++v) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) best[v] = fmaxf(best[v], __shfl_xor(best[v], o, 64));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) members += __shfl_xor(members, o, 64);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) s_sum[wave][k] = sum[k];
#pragma unroll
        for (int v = 0; v < TT_MAX_VIEWS; ++v) s_max[wave][v] = best[v];
        s_cnt[wave] = members;
    }
    __syncthreads();
    if (tid != 0) return;
    double tot[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        tot[k] = s_sum[0][k];
#pragma unroll
        for (int w = 1; w < TT_VOTE_WAVES; ++w) tot[k] += s_sum[w][k];
    }
    int cnt = 0;
#pragma unroll
    for (int w = 0; w < TT_VOTE_WAVES; ++w) cnt += s_cnt[w];
    float o[7];
    if (tot[0] > 0.0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = (float)(tot[1 + k] / tot[0]);
        o[6] = (float)(qi[6] + tot[7] / tot[0]);
    } else {          // no weight to divide by: the kept row as it is
#pragma unroll
        for (int k = 0; k < 7; ++k) o[k] = bx[(size_t)i * 7 + k];
    }
    float score = sc[i];
    if (score_mode == VN_VOTE_S_VIEW_MEAN) {
        double acc = 0.0;
#pragma unroll
        for (int v = 0; v < TT_MAX_VIEWS; ++v) {
            float mx = s_max[0][v];
#pragma unroll
            for (int w = 1; w < TT_VOTE_WAVES; ++w) mx = fmaxf(mx, s_max[w][v]);
            if (v < V) acc += mx == -INFINITY ? 0.0 : (double)mx;          // a view without a member counts 0
        }
        score = (float)(acc / (double)V);
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) w_boxes[slot * 7 + k] = o[k];
    w_scores[slot] = score;
    w_members[slot] = cnt;
    w_valid[slot] = 1;
}

__global__ void __launch_bounds__(VN_WAVE) k_tta_vote_order(const int32_t *__restrict__ keep_counts, int P,
                                                           const float *__restrict__ w_boxes, const float *__restrict__ w_scores,
                                                           const int32_t *__restrict__ w_members, const int32_t *__restrict__ w_valid,
                                                           float *__restrict__ out_boxes, float *__restrict__ out_scores,
                                                           int32_t *__restrict__ out_members, int32_t *__restrict__ out_counts) {
    __shared__ uint64_t skey[VN_WAVE];
    const int b = blockIdx.x, t = threadIdx.x;
    const int m = min(max(keep_counts[b], 0), P);
    const size_t slot = (size_t)b * P + t;
    const bool valid = t < m && w_valid[slot] != 0;
    uint64_t key = 0;          // a skipped entry; a valid one is > 0 (~t != 0), a NaN score behind every number
    float score = 0.0f;
    if (valid) {
        score = w_scores[slot];
        key = ((uint64_t)(score == score ? tt_score_bits(score) : 0u) << 32) | (uint32_t)~(uint32_t)t;
    }
    skey[t] = key;
    __syncthreads();
    int rank = 0;
    for (int u = 0; u < VN_WAVE; ++u) rank += skey[u] > key ? 1 : 0;
    const uint64_t vm = __ballot(valid);
    if (t == 0) out_counts[b] = __popcll((unsigned long long)vm);
    if (!valid) return;
    const size_t out = (size_t)b * P + rank;
#pragma unroll
    for (int k = 0; k < 7; ++k) out_boxes[out * 7 + k] = w_boxes[slot * 7 + k];
    out_scores[out] = score;
    out_members[out] = w_members[slot];
}

inline bool tt_finite(double v) { return v - v == 0.0; }

inline bool tt_merge_ok(int32_t V, int32_t B, int32_t K) {
    return V >= 1 && V <= TT_MAX_VIEWS && B >= 1 && B <= (1 << 20) && K >= 1 && (int64_t)V * K <= TT_MAX_ROWS;
}
inline bool tt_vote_ok(int32_t B, int32_t K, int32_t P, int32_t V) {
    return B >= 1 && B <= 65535 /* grid.y */ && K >= 1 && K <= TT_MAX_ROWS && P >= 1 && P <= TT_MAX_KEEP && V >= 1 && V <= TT_MAX_VIEWS;
}

}  // namespace

// Reserved: the merge keeps its keys in LDS and takes the view table as a kernel argument, so nothing is stored here today;
// the query still answers 0 for sizes the call refuses, like every other one.
extern "C" size_t vn_pool_merge_workspace_bytes(int32_t V, int32_t B, int32_t K) {
    return tt_merge_ok(V, B, K) ? vn_align(1) : 0;
}

extern "C" int vn_pool_merge(const float *boxes, const float *scores, const int32_t *counts, const double *views, int32_t V, int32_t B,
                             int32_t K, float *out_boxes, float *out_scores, int32_t *out_src, int32_t *out_counts, void *workspace,
                             size_t workspace_bytes, vnStream stream) {
    VN_CHECK_ARG(boxes && scores && counts && views && out_boxes && out_scores && out_src && out_counts && workspace);
    VN_CHECK_ARG(tt_merge_ok(V, B, K));
    TtViews tv = {};
    for (int v = 0; v < V; ++v) {
        const double fy = views[3 * v], angle = views[3 * v + 1], factor = views[3 * v + 2];
        VN_CHECK_ARG((fy == 1.0 || fy == -1.0) && tt_finite(angle) && tt_finite(factor) && factor > 0.0);
        tv.fy[v] = fy;
        tv.c[v] = cos(angle);
        tv.s[v] = sin(angle);
        tv.angle[v] = angle;
        tv.factor[v] = factor;
        tv.identity[v] = (fy == 1.0 && angle == 0.0 && factor == 1.0) ? 1 : 0;
    }
    if (workspace_bytes < vn_pool_merge_workspace_bytes(V, B, K)) return VN_EWORKSPACE;
    k_tta_merge<<<B, TT_MERGE_THREADS, 0, vn_stream(stream)>>>(boxes, scores, counts, tv, V, B, K, out_boxes, out_scores, out_src,
                                                               out_counts);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

// workspace of vn_box_vote: [fields B*P*7 f32 | scores B*P f32 | members B*P i32 | valid B*P i32]
extern "C" size_t vn_box_vote_workspace_bytes(int32_t B, int32_t K, int32_t P, int32_t V) {
    if (!tt_vote_ok(B, K, P, V)) return 0;
    const size_t rows = (size_t)B * P;
    return vn_align(rows * 7 * sizeof(float)) + vn_align(rows * sizeof(float)) + 2 * vn_align(rows * sizeof(int32_t));
}

extern "C" int vn_box_vote(const float *boxes, const float *scores, const int32_t *counts, const int32_t *src, int32_t rows_per_view,
                           const int32_t *keep_idx, const int32_t *keep_counts, int32_t B, int32_t K, int32_t P, int32_t V,
                           double vote_thres, int32_t weight_mode, int32_t score_mode, float *out_boxes, float *out_scores,
                           int32_t *out_members, int32_t *out_counts, void *workspace, size_t workspace_bytes, vnStream stream) {
    VN_CHECK_ARG(boxes && scores && counts && keep_idx && keep_counts && out_boxes && out_scores && out_members && out_counts &&
                 workspace);
    VN_CHECK_ARG(tt_vote_ok(B, K, P, V) && tt_finite(vote_thres) && vote_thres > 0.0);
    VN_CHECK_ARG(weight_mode == VN_VOTE_W_SCORE || weight_mode == VN_VOTE_W_SCORE_IOU);
    VN_CHECK_ARG(score_mode == VN_VOTE_S_KEEP || score_mode == VN_VOTE_S_VIEW_MEAN);
    VN_CHECK_ARG(src ? rows_per_view >= 1 : V == 1);
    if (workspace_bytes < vn_box_vote_workspace_bytes(B, K, P, V)) return VN_EWORKSPACE;
    hipStream_t st = vn_stream(stream);
    const size_t rows = (size_t)B * P;
    char *p = static_cast<char *>(workspace);
    float *w_boxes = reinterpret_cast<float *>(p);       p += vn_align(rows * 7 * sizeof(float));
    float *w_scores = reinterpret_cast<float *>(p);      p += vn_align(rows * sizeof(float));
    int32_t *w_members = reinterpret_cast<int32_t *>(p); p += vn_align(rows * sizeof(int32_t));
    int32_t *w_valid = reinterpret_cast<int32_t *>(p);
    k_tta_vote<<<dim3((unsigned)P, (unsigned)B), TT_VOTE_THREADS, 0, st>>>(boxes, scores, counts, src, rows_per_view, keep_idx,
                                                                           keep_counts, K, P, V, vote_thres, weight_mode, score_mode,
                                                                           w_boxes, w_scores, w_members, w_valid);
    VN_LAUNCH_STATUS();
    k_tta_vote_order<<<B, VN_WAVE, 0, st>>>(keep_counts, P, w_boxes, w_scores, w_members, w_valid, out_boxes, out_scores, out_members,
                                            out_counts);
    VN_LAUNCH_STATUS();
    return VN_OK;
}
