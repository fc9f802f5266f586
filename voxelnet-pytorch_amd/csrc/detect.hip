// Detection tail for evaluation: what predict.hip does for the reference's 20-candidate tail
// (filter_boxes model.py:28-57, deltas_to_boxes_3d utils.py:476-489, utils.nms utils.py:492-553), widened to the three
// steps an average precision needs — a pre-NMS top-K in the thousands, a greedy NMS on stand-up rectangles or on the
// ROTATED footprints, a post-NMS cap.  vn_rpn_predict itself is untouched.
//
//   k_dt_filter   one thread per anchor: the candidates p >= score_thres as unique 64-bit keys
//                 (order-preserving map of the score's bits | flat index), slots handed out by an atomic.
//   k_dt_select   one workgroup per sample: the pre_top_k-th largest key by radix passes (8 bits each, most significant
//                 first) over an LDS histogram, compaction of the keys at or above it into LDS, a bitonic sort there
//                 (<= 4096 x 8 B = 32 KB), then the decoding of the selected rows by the codec k_pr_select_nms uses (rpn_common.h).
//                 The keys are unique, so neither the selected set nor its order depends on the atomics' order.
//   k_dt_nms      one workgroup per sample, LAZY: the walk ends at <= 64 kept rows, so only <= 64 x K pairs are ever
//                 evaluated (a K x K suppression matrix would be 8.4 M clippings at K = 4096).  Per kept row every
//                 thread tests its own still-alive later rows (row = q * 512 + thread: the later rows stay spread over
//                 all threads) and the workgroup agrees on the next alive row by a ballot per wave and an 8-entry LDS
//                 reduction.  Rotated mode: (x, y, half-diagonal) of every row sit in LDS (48 KB); a pair whose centres
//                 are further apart than the two half-diagonals together has disjoint footprints, the pair function
//                 returns exactly 0 for it, and it is skipped without clipping (only for nms_thres >= 0: 0 <= thres
//                 keeps); full rows come from L2 for the near pairs only.  512 threads = 2 waves per SIMD: the clipping
//                 (~130 VGPRs, common.h box_iou_pair) does not spill.
//   k_dt_gather   the kept rows in vn_rpn_predict's output format.
// Layout: k_dt_filter and the decode of k_dt_select are templates on how the maps are read —
// VN_DETECT_FLAT, the reference's reshape without a permute, or VN_DETECT_SITE, anchor n = 2 * site + a from probs[b, a, site]
// and deltas[b, 7a .. 7a+6, site], the layout the loss trains.  The index in the key, in sel_idx and into `anchors` is n.
// Equal scores: the larger flat index first (predict.hip, oracle/predict.py); -0.0 and +0.0 are one score; a NaN score
// fails `p >= thres` and is never a candidate.
#include "rpn_common.h"

namespace {

constexpr int DT_FILTER_THREADS = 256;
constexpr int DT_SEL_THREADS = 1024;
constexpr int DT_NMS_THREADS = 512;
constexpr int DT_MAX_PRE = VN_DETECT_MAX_PRE;
constexpr int DT_MAX_POST = VN_PREDICT_MAX_TOPK;
constexpr int DT_ROWS = DT_MAX_PRE / DT_NMS_THREADS;          // rows of one thread in the walk
constexpr int DT_NONE = 0x7fffffff;

static_assert(DT_MAX_PRE % DT_NMS_THREADS == 0 && DT_ROWS <= 32, "a thread's alive rows are the bits of one register");
static_assert((DT_MAX_PRE & (DT_MAX_PRE - 1)) == 0, "the bitonic network sorts a power of two");
static_assert(DT_MAX_PRE * sizeof(uint64_t) + 1024 + 64 <= 65536, "keys + histogram fit the 64 KB of LDS a launch gets by default");
static_assert(3 * DT_MAX_PRE * sizeof(float) + 256 <= 65536, "(x, y, half-diagonal) of every row fit it too");
static_assert(DT_MAX_POST <= DT_NMS_THREADS, "one thread per output slot");

// (score, flat index) -> a unique key whose unsigned order is the lexicographic order of (score, index)
__device__ __forceinline__ uint64_t dt_key(float p, int j) {
    uint32_t u = p == 0.0f ? 0u : __float_as_uint(p);          // -0.0 == +0.0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint32_t)j;
}

// SITE (VN_DETECT_SITE): flat element j = a * S + s of probs[b] is anchor n = 2 * s + a (S = N / 2 sites,
// rotation a); the threads still walk the map in memory order, only the index in the key changes
template <bool SITE>
__global__ void __launch_bounds__(DT_FILTER_THREADS) k_dt_filter(const float *__restrict__ probs, int N, float thres,
                                                                 int32_t *__restrict__ count, uint64_t *__restrict__ cand_key) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * DT_FILTER_THREADS + threadIdx.x;
    if (j >= N) return;
    const float p = probs[(size_t)b * N + j];
    if (p >= thres) {                                   // model.py:34; false for a NaN
        const int slot = atomicAdd(count + b, 1);        // order irrelevant: the keys are unique
        const int S = N >> 1;
        const int n = SITE ? (j >= S ? 2 * (j - S) + 1 : 2 * j) : j;
        cand_key[(size_t)b * N + slot] = dt_key(p, n);
    }
}

template <bool SITE>
__global__ void __launch_bounds__(DT_SEL_THREADS) k_dt_select(const float *__restrict__ probs, const float *__restrict__ deltas,
                                                              const double *__restrict__ anchors, int N,
                                                              const int32_t *__restrict__ count,
                                                              const uint64_t *__restrict__ cand_key, int pre_k, double anchor_h,
                                                              float *__restrict__ sel_boxes, float *__restrict__ sel_scores,
                                                              int32_t *__restrict__ sel_idx, int32_t *__restrict__ sel_counts) {
    __shared__ uint64_t skey[DT_MAX_PRE];
    __shared__ uint32_t hist[256];
    __shared__ uint64_t s_prefix;
    __shared__ int s_krem, s_done, s_fill;
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = min(max(count[b], 0), N);
    const int n_sel = min(M, pre_k);
    const uint64_t *ck = cand_key + (size_t)b * N;
    if (M <= pre_k) {
        for (int c = tid; c < M; c += DT_SEL_THREADS) skey[c] = ck[c];
    } else {
        // ---- the pre_k-th largest key: after the pass at `shift`, `prefix` = its bits from `shift` upwards and krem =
        // its rank among the keys that share them
        uint64_t prefix = 0;
        int krem = pre_k, shift = 56;
        for (int pass = 0; pass < 8; ++pass) {
            shift = 56 - 8 * pass;
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int base = 0; base < M; base += DT_SEL_THREADS) {          // workgroup-uniform trip count: the ballots are whole
                const int c = base + tid;
                const uint64_t key = c < M ? ck[c] : 0;
                const bool act = c < M && (pass == 0 || (key >> (shift + 8)) == prefix);
                const int d = (int)((key >> shift) & 255);
                const uint64_t am = __ballot(act);
                if (am) {          // a wave whose candidates share the digit (the exponent byte of scores in [0.5, 1)) adds once
                    const int first = __ffsll((unsigned long long)am) - 1;
                    const int d0 = __shfl(d, first, 64);
                    const uint64_t same = __ballot(act && d == d0);
                    if (same == am) {
                        if (lane == first) atomicAdd(&hist[d0], (uint32_t)__popcll(am));
                    } else if (act) {
                        atomicAdd(&hist[d], 1u);
                    }
                }
            }
            __syncthreads();
            if (wave == 0) {          // bins from 255 downwards, four per lane: the bin that holds rank krem
                const int top = 255 - 4 * lane;
                const int h0 = (int)hist[top], h1 = (int)hist[top - 1], h2 = (int)hist[top - 2], h3 = (int)hist[top - 3];
                const int s = h0 + h1 + h2 + h3;
                int inc = s;
                for (int o = 1; o < 64; o <<= 1) {
                    const int v = __shfl_up(inc, o, 64);
                    if (lane >= o) inc += v;
                }
                int before = inc - s;
                if (before < krem && krem <= inc) {          // exactly one lane
                    int d = top, cnt = h0;
                    if (krem > before + h0) {
                        before += h0; d = top - 1; cnt = h1;
                        if (krem > before + h1) {
                            before += h1; d = top - 2; cnt = h2;
                            if (krem > before + h2) { before += h2; d = top - 3; cnt = h3; }
                        }
                    }
                    s_prefix = (prefix << 8) | (uint64_t)d;
                    s_krem = krem - before;
                    s_done = (cnt == krem - before) ? 1 : 0;          // every key with this prefix is taken: the lower bits are free
                }
            }
            __syncthreads();
            prefix = s_prefix;
            krem = s_krem;
            if (s_done) break;
        }
        const uint64_t thr = prefix << shift;
        if (tid == 0) s_fill = 0;
        __syncthreads();
        for (int c = tid; c < M; c += DT_SEL_THREADS) {
            const uint64_t key = ck[c];
            if (key >= thr) {
                const int slot = atomicAdd(&s_fill, 1);
                if (slot < DT_MAX_PRE) skey[slot] = key;          // (exactly pre_k keys qualify)
            }
        }
        __syncthreads();
        for (int c = s_fill + tid; c < n_sel; c += DT_SEL_THREADS) skey[c] = 0;          // never taken: no slot is left unwritten
    }
    // ---- descending bitonic sort of the n_sel keys, padded with 0 (below every key: a candidate's high word is > 0)
    int P = 1;
    while (P < n_sel) P <<= 1;
    for (int c = n_sel + tid; c < P; c += DT_SEL_THREADS) skey[c] = 0;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += DT_SEL_THREADS) {
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
    // ---- decode the selected rows (utils.py:476-489)
    for (int t = tid; t < n_sel; t += DT_SEL_THREADS) {
        const int j = (int)(uint32_t)(skey[t] & 0xffffffffull);
        if (j >= N) continue;
        // FLAT: seven consecutive elements; SITE: anchor j = 2 * s + a reads channels 7a .. 7a+6 at site s (stride S)
        const int S = N >> 1;
        const size_t d0 = SITE ? (size_t)b * N * 7 + (size_t)(j & 1) * 7 * S + (j >> 1) : ((size_t)b * N + j) * 7;
        const size_t ds = SITE ? (size_t)S : 1;
        float d[7], o[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) d[k] = deltas[d0 + k * ds];
        vn_box_decode_f32(d, anchors + (size_t)j * 7, anchor_h, o);
#pragma unroll
        for (int k = 0; k < 7; ++k) sel_boxes[((size_t)b * pre_k + t) * 7 + k] = o[k];
        sel_scores[(size_t)b * pre_k + t] = probs[(size_t)b * N + (SITE ? (size_t)(j & 1) * S + (j >> 1) : (size_t)j)];
        sel_idx[(size_t)b * pre_k + t] = j;
    }
    if (tid == 0) sel_counts[b] = n_sel;
}

// the lowest alive row of the workgroup (DT_NONE: none).  Row q * DT_NMS_THREADS + tid is bit q of the thread's `alive`.
__device__ __forceinline__ int dt_next_alive(unsigned alive, int lane, int wave, int (&wmin)[2][DT_NMS_THREADS / 64], int &par) {
    int m = DT_NONE;
    for (int q = 0; q < DT_ROWS; ++q) {
        const uint64_t mask = __ballot((alive >> q) & 1u);
        if (mask) {
            m = q * DT_NMS_THREADS + wave * 64 + (__ffsll((unsigned long long)mask) - 1);
            break;
        }
    }
    if (lane == 0) wmin[par][wave] = m;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < DT_NMS_THREADS / 64; ++w) m = min(m, wmin[par][w]);
    par ^= 1;          // the next call writes the other buffer: one barrier per call is enough
    return m;
}

template <int MODE>
__global__ void __launch_bounds__(DT_NMS_THREADS) k_dt_nms(const float *__restrict__ boxes, const int32_t *__restrict__ counts, int K,
                                                           double nms_thres, int post_k, float *__restrict__ rects,
                                                           int32_t *__restrict__ keep_idx, int32_t *__restrict__ keep_counts) {
    constexpr int NL = MODE == VN_NMS_ROTATED ? DT_MAX_PRE : 1;
    __shared__ float sx[NL], sy[NL], shd[NL];
    __shared__ int wmin[2][DT_NMS_THREADS / 64];
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(counts[b], 0), K);
    const float *bx = boxes + (size_t)b * K * 7;
    float *rc = rects + (size_t)b * K * 4;
    const bool reject_far = nms_thres >= 0.0;
    unsigned alive = 0;
    for (int q = 0; q < DT_ROWS; ++q) {
        const int j = q * DT_NMS_THREADS + tid;
        if (j >= n) break;
        float o[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) o[k] = bx[(size_t)j * 7 + k];
        if (MODE == VN_NMS_ROTATED) {
            double qd[7];
#pragma unroll
            for (int k = 0; k < 7; ++k) qd[k] = (double)o[k];
            const bool ok = box_ok(qd);          // an invalid row is never kept and suppresses nothing
            sx[j] = o[0];
            sy[j] = o[1];
            // the footprint lies within this distance of the centre; the factor covers the rounding to float32
            shd[j] = ok ? (float)(0.5 * sqrt(qd[4] * qd[4] + qd[5] * qd[5]) * 1.000001) : 0.0f;
            if (ok) alive |= 1u << q;
        } else {
            float r[4];
            vn_box_standup_f32(o, r);
#pragma unroll
            for (int k = 0; k < 4; ++k) rc[(size_t)j * 4 + k] = r[k];          // read back by this thread only
            alive |= 1u << q;
        }
    }
    __syncthreads();
    int par = 0, kept = 0;
    int cur = dt_next_alive(alive, lane, wave, wmin, par);
    while (cur < n) {          // cur is workgroup-uniform
        if (tid == 0) keep_idx[(size_t)b * post_k + kept] = cur;
        ++kept;
        if (kept == post_k) break;
        float oi[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) oi[k] = bx[(size_t)cur * 7 + k];
        double qa[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) qa[k] = (double)oi[k];
        float ri[4] = {0.f, 0.f, 0.f, 0.f};
        double xi = 0.0, yi = 0.0, hi = 0.0, ai = 0.0;
        if (MODE == VN_NMS_ROTATED) {
            xi = (double)sx[cur]; yi = (double)sy[cur]; hi = (double)shd[cur];
        } else {
            vn_box_standup_f32(oi, ri);
            ai = ((double)ri[2] - (double)ri[0]) * ((double)ri[3] - (double)ri[1]);
        }
#pragma unroll 1
        for (int q = 0; q < DT_ROWS; ++q) {
            if (!((alive >> q) & 1u)) continue;
            const int j = q * DT_NMS_THREADS + tid;
            if (j <= cur) { alive &= ~(1u << q); continue; }          // the kept row itself
            bool dead;
            if (MODE == VN_NMS_ROTATED) {
                const double dx = (double)sx[j] - xi, dy = (double)sy[j] - yi, r = (double)shd[j] + hi;
                if (reject_far && dx * dx + dy * dy > r * r) continue;          // disjoint footprints: IoU exactly 0 <= thres
                double qb[7];
#pragma unroll
                for (int k = 0; k < 7; ++k) qb[k] = (double)bx[(size_t)j * 7 + k];
                double bev, v3;
                box_iou_pair(qa, qb, bev, v3);
                dead = !(bev <= nms_thres);
            } else {
                const double u0 = rc[(size_t)j * 4 + 0], u1 = rc[(size_t)j * 4 + 1], u2 = rc[(size_t)j * 4 + 2], u3 = rc[(size_t)j * 4 + 3];
                const double t0 = ri[0], t1 = ri[1], t2 = ri[2], t3 = ri[3];
                const double xx1 = fmax(u0, t0), yy1 = fmax(u1, t1);
                const double xx2 = fmin(u2, t2), yy2 = fmin(u3, t3);
                const double w = fmax(xx2 - xx1, 0.0), h = fmax(yy2 - yy1, 0.0);
                const double inter = w * h;
                const double au = (u2 - u0) * (u3 - u1);
                const double iou = inter / ((au - inter) + ai);
                dead = !(iou <= nms_thres);          // IoU.le(overlap) keeps; NaN does not
            }
            if (dead) alive &= ~(1u << q);
        }
        cur = dt_next_alive(alive, lane, wave, wmin, par);
    }
    if (tid == 0) keep_counts[b] = kept;
    if (tid >= kept && tid < post_k) keep_idx[(size_t)b * post_k + tid] = -1;
}

__global__ void __launch_bounds__(64) k_dt_gather(const float *__restrict__ sel_boxes, const float *__restrict__ sel_scores, int pre_k,
                                                  const int32_t *__restrict__ keep_idx, const int32_t *__restrict__ keep_counts,
                                                  int post_k, float *__restrict__ boxes, float *__restrict__ scores,
                                                  int32_t *__restrict__ counts) {
    const int b = blockIdx.x, t = threadIdx.x;
    const int kept = min(max(keep_counts[b], 0), post_k);
    if (t == 0) counts[b] = kept;
    if (t >= kept) return;
    const int r = keep_idx[(size_t)b * post_k + t];
    if (r < 0 || r >= pre_k) return;
#pragma unroll
    for (int k = 0; k < 7; ++k) boxes[((size_t)b * post_k + t) * 7 + k] = sel_boxes[((size_t)b * pre_k + r) * 7 + k];
    scores[(size_t)b * post_k + t] = sel_scores[(size_t)b * pre_k + r];
}

inline bool dt_select_ok(int32_t B, int32_t N, int32_t pre_k) {
    return B > 0 && N > 0 && pre_k >= 1 && pre_k <= DT_MAX_PRE && (int64_t)B * N < (1ll << 31) / 8;
}
inline bool dt_nms_ok(int32_t B, int32_t K, int32_t post_k) {
    return B > 0 && B <= (1 << 20) && K >= 1 && K <= DT_MAX_PRE && post_k >= 1 && post_k <= DT_MAX_POST;
}
inline bool dt_finite(double v) { return v - v == 0.0; }

// workspace of vn_rpn_select_decode: [candidate counts | candidate keys]
inline size_t dt_sel_cnt_bytes(int32_t B) { return vn_align((size_t)B * sizeof(int32_t)); }

inline bool dt_layout_ok(int32_t layout, int32_t N) {
    return layout == VN_DETECT_FLAT || (layout == VN_DETECT_SITE && N % 2 == 0);
}

int dt_select(const float *probs, const float *deltas, const double *anchors, int32_t B, int32_t N, float score_thres, int32_t pre_k,
              double anchor_h, float *sel_boxes, float *sel_scores, int32_t *sel_idx, int32_t *sel_counts, char *ws, hipStream_t st,
              int32_t layout) {
    int32_t *cnt = reinterpret_cast<int32_t *>(ws);
    uint64_t *keys = reinterpret_cast<uint64_t *>(ws + dt_sel_cnt_bytes(B));
    VN_HIP(hipMemsetAsync(cnt, 0, (size_t)B * sizeof(int32_t), st));
    const dim3 grid((unsigned)((N + DT_FILTER_THREADS - 1) / DT_FILTER_THREADS), (unsigned)B);
    if (layout == VN_DETECT_SITE) {
        k_dt_filter<true><<<grid, DT_FILTER_THREADS, 0, st>>>(probs, N, score_thres, cnt, keys);
        VN_LAUNCH_STATUS();
        k_dt_select<true><<<B, DT_SEL_THREADS, 0, st>>>(probs, deltas, anchors, N, cnt, keys, pre_k, anchor_h, sel_boxes, sel_scores,
                                                       sel_idx, sel_counts);
    } else {
        k_dt_filter<false><<<grid, DT_FILTER_THREADS, 0, st>>>(probs, N, score_thres, cnt, keys);
        VN_LAUNCH_STATUS();
        k_dt_select<false><<<B, DT_SEL_THREADS, 0, st>>>(probs, deltas, anchors, N, cnt, keys, pre_k, anchor_h, sel_boxes, sel_scores,
                                                        sel_idx, sel_counts);
    }
    VN_LAUNCH_STATUS();
    return VN_OK;
}

int dt_nms(const float *boxes, const int32_t *counts, int32_t B, int32_t K, int32_t mode, double nms_thres, int32_t post_k,
           int32_t *keep_idx, int32_t *keep_counts, char *ws, hipStream_t st) {
    float *rects = reinterpret_cast<float *>(ws);
    if (mode == VN_NMS_ROTATED)
        k_dt_nms<VN_NMS_ROTATED><<<B, DT_NMS_THREADS, 0, st>>>(boxes, counts, K, nms_thres, post_k, rects, keep_idx, keep_counts);
    else
        k_dt_nms<VN_NMS_STANDUP><<<B, DT_NMS_THREADS, 0, st>>>(boxes, counts, K, nms_thres, post_k, rects, keep_idx, keep_counts);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

}  // namespace

extern "C" size_t vn_rpn_select_decode_workspace_bytes(int32_t B, int32_t n_anchors, int32_t pre_top_k) {
    if (!dt_select_ok(B, n_anchors, pre_top_k)) return 0;
    return dt_sel_cnt_bytes(B) + vn_align((size_t)B * n_anchors * sizeof(uint64_t));
}

extern "C" int vn_rpn_select_decode_layout(const float *probs, const float *deltas, const double *anchors, int32_t B,
                                           int32_t n_anchors, float score_thres, int32_t pre_top_k, double anchor_h, float *sel_boxes,
                                           float *sel_scores, int32_t *sel_idx, int32_t *sel_counts, void *workspace,
                                           size_t workspace_bytes, vnStream stream, int32_t layout) {
    VN_CHECK_ARG(probs && deltas && anchors && sel_boxes && sel_scores && sel_idx && sel_counts && workspace);
    VN_CHECK_ARG(dt_select_ok(B, n_anchors, pre_top_k) && dt_layout_ok(layout, n_anchors));
    if (workspace_bytes < vn_rpn_select_decode_workspace_bytes(B, n_anchors, pre_top_k)) return VN_EWORKSPACE;
    return dt_select(probs, deltas, anchors, B, n_anchors, score_thres, pre_top_k, anchor_h, sel_boxes, sel_scores, sel_idx, sel_counts,
                     static_cast<char *>(workspace), vn_stream(stream), layout);
}

extern "C" int vn_rpn_select_decode(const float *probs, const float *deltas, const double *anchors, int32_t B, int32_t n_anchors,
                                    float score_thres, int32_t pre_top_k, double anchor_h, float *sel_boxes, float *sel_scores,
                                    int32_t *sel_idx, int32_t *sel_counts, void *workspace, size_t workspace_bytes, vnStream stream) {
    return vn_rpn_select_decode_layout(probs, deltas, anchors, B, n_anchors, score_thres, pre_top_k, anchor_h, sel_boxes, sel_scores,
                                       sel_idx, sel_counts, workspace, workspace_bytes, stream, VN_DETECT_FLAT);
}

extern "C" size_t vn_box_nms_workspace_bytes(int32_t B, int32_t K) {
    if (!dt_nms_ok(B, K, 1)) return 0;
    return vn_align((size_t)B * K * 4 * sizeof(float));          // the stand-up rectangles
}

extern "C" int vn_box_nms(const float *boxes, const int32_t *counts, int32_t B, int32_t K, int32_t mode, double nms_thres,
                          int32_t post_top_k, int32_t *keep_idx, int32_t *keep_counts, void *workspace, size_t workspace_bytes,
                          vnStream stream) {
    VN_CHECK_ARG(boxes && counts && keep_idx && keep_counts && workspace);
    VN_CHECK_ARG(dt_nms_ok(B, K, post_top_k) && (mode == VN_NMS_STANDUP || mode == VN_NMS_ROTATED) && dt_finite(nms_thres));
    if (workspace_bytes < vn_box_nms_workspace_bytes(B, K)) return VN_EWORKSPACE;
    return dt_nms(boxes, counts, B, K, mode, nms_thres, post_top_k, keep_idx, keep_counts, static_cast<char *>(workspace),
                  vn_stream(stream));
}

// workspace of vn_rpn_detect: [select's | sel_boxes | sel_scores | sel_idx | sel_counts | keep_idx | keep_counts | nms's]
extern "C" size_t vn_rpn_detect_workspace_bytes(int32_t B, int32_t n_anchors, int32_t pre_top_k) {
    if (!dt_select_ok(B, n_anchors, pre_top_k) || !dt_nms_ok(B, pre_top_k, 1)) return 0;
    const size_t rows = (size_t)B * pre_top_k;
    return vn_rpn_select_decode_workspace_bytes(B, n_anchors, pre_top_k) + vn_align(rows * 7 * sizeof(float)) +
           vn_align(rows * sizeof(float)) + vn_align(rows * sizeof(int32_t)) + vn_align((size_t)B * sizeof(int32_t)) +
           vn_align((size_t)B * DT_MAX_POST * sizeof(int32_t)) + vn_align((size_t)B * sizeof(int32_t)) +
           vn_box_nms_workspace_bytes(B, pre_top_k);
}

extern "C" int vn_rpn_detect_layout(const float *probs, const float *deltas, const double *anchors, int32_t B, int32_t n_anchors,
                                    float score_thres, int32_t pre_top_k, int32_t mode, double nms_thres, int32_t post_top_k,
                                    double anchor_h, float *boxes, float *scores, int32_t *counts, void *workspace,
                                    size_t workspace_bytes, vnStream stream, int32_t layout) {
    VN_CHECK_ARG(probs && deltas && anchors && boxes && scores && counts && workspace);
    VN_CHECK_ARG(dt_select_ok(B, n_anchors, pre_top_k) && dt_nms_ok(B, pre_top_k, post_top_k) && dt_layout_ok(layout, n_anchors));
    VN_CHECK_ARG((mode == VN_NMS_STANDUP || mode == VN_NMS_ROTATED) && dt_finite(nms_thres));
    if (workspace_bytes < vn_rpn_detect_workspace_bytes(B, n_anchors, pre_top_k)) return VN_EWORKSPACE;
    hipStream_t st = vn_stream(stream);
    const size_t rows = (size_t)B * pre_top_k;
    char *ws = static_cast<char *>(workspace);
    char *p = ws + vn_rpn_select_decode_workspace_bytes(B, n_anchors, pre_top_k);
    float *sel_boxes = reinterpret_cast<float *>(p);      p += vn_align(rows * 7 * sizeof(float));
    float *sel_scores = reinterpret_cast<float *>(p);     p += vn_align(rows * sizeof(float));
    int32_t *sel_idx = reinterpret_cast<int32_t *>(p);    p += vn_align(rows * sizeof(int32_t));
    int32_t *sel_counts = reinterpret_cast<int32_t *>(p); p += vn_align((size_t)B * sizeof(int32_t));
    int32_t *keep_idx = reinterpret_cast<int32_t *>(p);   p += vn_align((size_t)B * DT_MAX_POST * sizeof(int32_t));
    int32_t *keep_counts = reinterpret_cast<int32_t *>(p); p += vn_align((size_t)B * sizeof(int32_t));
    int rc = dt_select(probs, deltas, anchors, B, n_anchors, score_thres, pre_top_k, anchor_h, sel_boxes, sel_scores, sel_idx,
                       sel_counts, ws, st, layout);
    if (rc != VN_OK) return rc;
    rc = dt_nms(sel_boxes, sel_counts, B, pre_top_k, mode, nms_thres, post_top_k, keep_idx, keep_counts, p, st);
    if (rc != VN_OK) return rc;
    k_dt_gather<<<B, 64, 0, st>>>(sel_boxes, sel_scores, pre_top_k, keep_idx, keep_counts, post_top_k, boxes, scores, counts);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" int vn_rpn_detect(const float *probs, const float *deltas, const double *anchors, int32_t B, int32_t n_anchors,
                             float score_thres, int32_t pre_top_k, int32_t mode, double nms_thres, int32_t post_top_k,
                             double anchor_h, float *boxes, float *scores, int32_t *counts, void *workspace, size_t workspace_bytes,
                             vnStream stream) {
    return vn_rpn_detect_layout(probs, deltas, anchors, B, n_anchors, score_thres, pre_top_k, mode, nms_thres, post_top_k, anchor_h,
                                boxes, scores, counts, workspace, workspace_bytes, stream, VN_DETECT_FLAT);
}
