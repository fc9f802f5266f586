// Shared by the four target assigners — targets.hip, targets_iou.hip, targets_atss.hip, targets_ota.hip — and by nothing
// else: the ONE copy of the IoU of an (anchor, box) pair, of the bounded per-lane lists and their wave merge, of the kernels
// behind the per-anchor best word, of an assignment's write tail and of the workspace carving.
#pragma once
#include "rpn_common.h"

namespace {

// ---- the stand-up IoU of the target assignments (targets_iou.hip, targets_atss.hip) ----
// the axis-aligned hull of the rotated footprint of (x, y, ., ., w, l, r) as (x, y, half width hx, half height hy, area)
__device__ __forceinline__ void ti_hull(const double (&q)[7], double (&h)[5]) {
    const double c = fabs(cos(q[6])), s = fabs(sin(q[6]));
    h[0] = q[0]; h[1] = q[1];
    h[2] = (q[5] * c + q[4] * s) / 2;
    h[3] = (q[5] * s + q[4] * c) / 2;
    h[4] = (2.0 * h[2]) * (2.0 * h[3]);
}

// The overlap of [xa - ha, xa + ha] and [xg - hg, xg + hg] written from the centres: min(ha + hg - |xg - xa|, 2 min(ha, hg)).
// Where one interval contains the other the second term is taken, which does not depend on the position: the anchors of a
// row that all contain a box's hull along x (or lie inside it) get THE SAME IoU bit for bit, not values that differ by the
// rounding of x +- ha, and the smallest index wins the tie in every implementation that writes the overlap this way.
__device__ __forceinline__ double ti_standup_iou(const double (&a)[5], const double *__restrict__ g) {
    const double iw = fmin((a[2] + g[2]) - fabs(g[0] - a[0]), 2.0 * fmin(a[2], g[2]));
    const double ih = fmin((a[3] + g[3]) - fabs(g[1] - a[1]), 2.0 * fmin(a[3], g[3]));
    if (!(iw > 0.0) || !(ih > 0.0)) return 0.0;
    const double inter = iw * ih;
    const double v = inter / ((a[4] + g[4]) - inter);
    return v > 0.0 ? v : 0.0;          // (a NaN from infinite extents is 0)
}

// ---- v(n,k), the IoU of an (anchor, box) pair under VN_ASSIGN_STANDUP / VN_ASSIGN_ROTATED: what vn_rpn_targets_iou assigns
// by and, bit for bit, what vn_rpn_targets_atss ranks its candidates by (k_ti_pairs, k_as_pick) ----
// What the pair function wants of each side beforehand.  Stand-up: ti_hull's five.  Rotated: [0] = the half-diagonal, a
// hair long (k_dt_nms's reject), < 0 for a box that fails box_ok; the other four are not touched.
template <int KIND> constexpr int ti_side_len() { return KIND == VN_ASSIGN_STANDUP ? 5 : 1; }
template <int KIND>
__device__ __forceinline__ void ti_pair_side(const double (&q)[7], double (&h)[5]) {
    if (KIND == VN_ASSIGN_STANDUP) ti_hull(q, h);
    else h[0] = box_ok(q) ? 0.5 * sqrt(q[4] * q[4] + q[5] * q[5]) * 1.000001 : -1.0;
}
// a, g: the anchor and the box (g, gh may point into LDS); ah, gh: their ti_pair_side.  -> whether v(n,k) > 0, and only then v.
// Rotated: an invalid box is 0; a pair whose centres are further apart than the two half-diagonals together has disjoint
// footprints, box_iou_pair returns exactly 0 for it, and it is left without clipping or reading the rest of g.
template <int KIND>
__device__ __forceinline__ bool ti_pair_iou(const double (&a)[7], const double (&ah)[5], const double *g, const double *gh, double &v) {
    if (KIND == VN_ASSIGN_STANDUP) return (v = ti_standup_iou(ah, gh)) > 0.0;
    const double hd = gh[0], hd_a = ah[0];
    if (hd_a < 0.0 || hd < 0.0) return false;
    const double dx = g[0] - a[0], dy = g[1] - a[1], r = hd + hd_a;
    if (dx * dx + dy * dy > r * r) return false;
    double q[7], v3;
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = g[j];
    box_iou_pair(a, q, v, v3);
    return v > 0.0;
}

// ---- the per-box assignments (targets_atss.hip, targets_ota.hip): bounded per-lane lists merged by wave
// arg-min rounds, an integer-atomic arg-best over the boxes' recorded candidates, one encode ----
constexpr int AS_MAX_CHUNKS = VN_WAVE;           // the per-box merge: one lane per chunk
constexpr int AS_MIN_CHUNK = 64;                 // sites of a chunk, at least (but for the last)
constexpr int AS_TARGET_WGS = 1024;              // the scan: workgroups wanted (256 CUs x 3 resident, and a tail)
constexpr int AS_ENC_THREADS = 256;
constexpr int AS_NONE = 0x7fffffff;              // the index of a list's padding: behind every anchor at +inf

// One round of a wave's lexicographic arg-min: every lane leaves with the smallest (d, n) of the 64.
__device__ __forceinline__ void as_wave_min(double &d, int &n) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(d, o, VN_WAVE);
        const int on = __shfl_xor(n, o, VN_WAVE);
        if (od < d || (od == d && on < n)) { d = od; n = on; }
    }
}

// A lane's bounded sorted list in LDS — the kernel declares the arrays: entry j of lane t at key[j][t], lanes on consecutive
// banks —: the `cap` smallest (key, id) of what the lane has offered, ascending; c = entries held, worst = the cap-th key
// once the list is full (+inf before), both in registers, so an offer that does not enter costs one compare.  The ids a lane
// offers GROW (n grows along its scan), so an offer whose key EQUALS an entry's ranks behind it: strict compares keep the
// (key, id) order exact.  Without id: a list of keys alone (equal keys need no order there) — by the argument's TYPE: a test of
// a pointer into LDS against null stays in the shift loop as a test at run time.
struct AsKeysAlone {};
template <int CAP, int LANES, typename ID = AsKeysAlone>
__device__ __forceinline__ void as_list_insert(double (&key)[CAP][LANES], int t, int cap, int &c, double &worst, double k, ID &&id = {},
                                               int32_t n = 0) {
    constexpr bool ids = !std::is_same<ID, AsKeysAlone>::value;
    if (!(c < cap || k < worst)) return;
    int j = min(c, cap - 1);
    while (j > 0 && key[j - 1][t] > k) {
        key[j][t] = key[j - 1][t];
        if constexpr (ids) id[j][t] = id[j - 1][t];
        --j;
    }
    key[j][t] = k;
    if constexpr (ids) id[j][t] = n;
    c = min(c + 1, cap);
    if (c == cap) worst = key[cap - 1][t];
}

// One round of a wave's merge of its 64 sorted lists (as_list_insert's, or ranked lists loaded one per lane): the arg-min over
// the heads; the lane that held it moves to its next entry; every lane returns the winning (key, id).  R rounds rank the R
// smallest of all the lists exactly, no barrier.  live: the lane has a list; len: its entries; a lane without a head offers
// the padding (+inf, AS_NONE), which is what a dry round returns.  Ties: with ids the smaller id — anchor indices are unique,
// exactly one lane advances —; without (keys alone, any of the equal ones will do) the smaller `lane`: the pick is unique.
struct AsHead { double key; int id; };
template <int CAP, int LANES, typename ID = AsKeysAlone>
__device__ __forceinline__ AsHead as_merge_round(const double (&key)[CAP][LANES], int t, int lane, bool live, int len, int &head,
                                                 ID &&id = {}) {
    const bool have = live && head < len;
    int mine = lane;
    if constexpr (!std::is_same<ID, AsKeysAlone>::value) mine = id[min(head, CAP - 1)][t];
    if (!have) mine = AS_NONE;
    AsHead m = {have ? key[min(head, CAP - 1)][t] : INFINITY, mine};
    as_wave_min(m.key, m.id);
    if (have && mine == m.id) ++head;
    return m;
}

// whether an anchor's centre, (dx, dy) from box q's, lies inside q's bird's-eye footprint, edges inside: u along the box's
// length l, w' along its width w; cr, sr = cos, sin of q's yaw
__device__ __forceinline__ bool as_in_footprint(double dx, double dy, double cr, double sr, const double (&q)[7]) {
    const double u = dx * cr + dy * sr, w = -(dx * sr) + dy * cr;
    return fabs(u) <= q[5] / 2 && fabs(w) <= q[4] / 2;
}

// The write tail of every assignment: pos, neg, matched (nullptr: not wanted) and the seven regression targets of anchor `a` at
// o = b * N + n, matched to box `box` (-1: none) of the boxes at gt_b.  is_neg is the caller's: the reference's may be both.
__device__ __forceinline__ void as_write_targets(size_t o, int box, bool is_neg, const double *gt_b, const double *a, double anchor_h,
                                                 float *pos, float *neg, float *targets, int32_t *matched) {
    pos[o] = box >= 0 ? 1.f : 0.f;
    neg[o] = is_neg ? 1.f : 0.f;
    if (matched) matched[o] = box;
    float t[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (box >= 0)
        vn_box_encode(gt_b + (size_t)box * 7, a, anchor_h, t);
#pragma unroll
    for (int j = 0; j < 7; ++j) targets[o * 7 + j] = t[j];
}

// A box's recorded candidates: SLOTS of (anchor n, bits), bits == 0 for an empty slot, else the value the box offered the
// anchor's best word by atomicMax.  Where the recorded bits equal the anchor's maximum — nothing is evaluated twice — an
// atomicMax on ~k leaves the smallest k.  (Templates, as rpn_common.h's k_pos_norm: only the files that launch them instantiate them.)
template <int SLOTS>
__global__ void __launch_bounds__(SLOTS) k_as_arg(int N, int max_gt, const unsigned long long *__restrict__ best_bits,
                                                  uint32_t *__restrict__ best_arg, const int32_t *__restrict__ cand_n,
                                                  const unsigned long long *__restrict__ cand_bits) {
    static_assert(SLOTS <= VN_WAVE, "one wave per box");
    const int k = blockIdx.x, b = blockIdx.y;
    const size_t ci = ((size_t)b * max_gt + k) * SLOTS + threadIdx.x;
    const unsigned long long bits = cand_bits[ci];
    if (!bits) return;
    const size_t o = (size_t)b * N + cand_n[ci];
    if (best_bits[o] == bits) atomicMax(best_arg + o, ~(uint32_t)k);
}

// stats[(b * max_gt + k) * stride + col] = the anchors matched to box k: its own recorded candidates (distinct anchors) that it
// won — no atomics
template <int SLOTS>
__global__ void __launch_bounds__(SLOTS) k_as_count(int N, int max_gt, const unsigned long long *__restrict__ best_bits,
                                                    const uint32_t *__restrict__ best_arg, const int32_t *__restrict__ cand_n,
                                                    const unsigned long long *__restrict__ cand_bits, double *__restrict__ stats,
                                                    int stride, int col) {
    static_assert(SLOTS <= VN_WAVE, "one wave per box");
    const int k = blockIdx.x, b = blockIdx.y;
    const size_t kb = (size_t)b * max_gt + k, ci = kb * SLOTS + threadIdx.x;
    const unsigned long long bits = cand_bits[ci];
    bool won = false;
    if (bits) {
        const size_t o = (size_t)b * N + cand_n[ci];
        won = best_bits[o] == bits && best_arg[o] == ~(uint32_t)k;
    }
    const unsigned long long m = __ballot(won);
    if (threadIdx.x == 0) stats[kb * stride + col] = (double)__popcll(m);
}

// matched, pos, neg and the seven regression targets of every anchor from its best word and its arg word
template <int THREADS>
__global__ void __launch_bounds__(THREADS) k_as_encode(const double *__restrict__ anchors, int N, const double *__restrict__ gt,
                                                       int max_gt, const unsigned long long *__restrict__ best_bits,
                                                       const uint32_t *__restrict__ best_arg, double anchor_h,
                                                       float *__restrict__ pos, float *__restrict__ neg,
                                                       float *__restrict__ targets, int32_t *__restrict__ matched) {
    const int b = blockIdx.y, n = blockIdx.x * THREADS + threadIdx.x;
    if (n >= N) return;
    const size_t o = (size_t)b * N + n;
    const int box = best_bits[o] ? (int)~best_arg[o] : -1;
    as_write_targets(o, box, box < 0, gt + (size_t)b * max_gt * 7, anchors + (size_t)n * 7, anchor_h, pos, neg, targets, matched);
}

// the limits of vn_rpn_targets and vn_rpn_targets_iou; the per-box assignments': an even anchor count too
inline bool tg_sizes_ok(int32_t B, int32_t N, int32_t max_gt) {
    return B > 0 && N > 0 && max_gt > 0 && max_gt <= VN_TARGETS_MAX_GT && (int64_t)B * N < (1ll << 31) / 8;
}
inline bool as_sizes_ok(int32_t B, int32_t N, int32_t max_gt) { return tg_sizes_ok(B, N, max_gt) && N % 2 == 0; }
// ranges the sites are cut into: AS_TARGET_WGS workgroups of the scan over the B * max_gt boxes, chunks of >= AS_MIN_CHUNK sites
inline int as_chunks(int32_t B, int32_t N, int32_t max_gt) {
    const int64_t want = AS_TARGET_WGS / ((int64_t)B * max_gt), fit = (N / 2 + AS_MIN_CHUNK - 1) / AS_MIN_CHUNK;
    return (int)std::max<int64_t>(1, std::min<int64_t>(std::min(want, fit), AS_MAX_CHUNKS));
}

// ---- an entry point's workspace: regions in the order they are added, each vn_align-ed.  The entry's own struct names them
// once — its constructor adds them; region(workspace) is the typed pointer — and yields both *_workspace_bytes and the pointers.
template <typename T> struct AsRegion {
    size_t off;
    T *operator()(void *ws) const { return reinterpret_cast<T *>(static_cast<char *>(ws) + off); }
};
struct AsLayout {
    size_t total = 0;
    template <typename T> AsRegion<T> add(size_t count) {
        const size_t off = total;
        total += vn_align(count * sizeof(T));
        return {off};
    }
    size_t bytes() const { return total; }
};

// The per-box assignments' workspace begins [best word of every anchor | ~k of every anchor | the boxes' recorded n | their bits]:
// the two dense words are adjacent so that one memset clears both; a box records `slots` candidates.
struct AsBoxWs : AsLayout {
    AsRegion<unsigned long long> best_bits, cand_bits;
    AsRegion<uint32_t> best_arg;
    AsRegion<int32_t> cand_n;
    size_t dense_bytes;
    AsBoxWs(int32_t B, int32_t N, int32_t max_gt, int slots) {
        best_bits = add<unsigned long long>((size_t)B * N);
        best_arg = add<uint32_t>((size_t)B * N);
        dense_bytes = total;
        cand_n = add<int32_t>((size_t)B * max_gt * slots);
        cand_bits = add<unsigned long long>((size_t)B * max_gt * slots);
    }
};

// What every per-box assignment ends with, once the boxes' candidates are recorded: the arg word, the anchors each box won into
// stats[..., col] (only with stats), the encode.
template <int SLOTS>
int as_launch_tail(const AsBoxWs &ws, void *w, hipStream_t st, const double *anchors, int N, const double *gt, int B, int max_gt,
                   double anchor_h, float *pos, float *neg, float *targets, int32_t *matched, double *stats, int stride, int col) {
    const dim3 boxes((unsigned)max_gt, (unsigned)B), grid((unsigned)((N + AS_ENC_THREADS - 1) / AS_ENC_THREADS), (unsigned)B);
    k_as_arg<SLOTS><<<boxes, SLOTS, 0, st>>>(N, max_gt, ws.best_bits(w), ws.best_arg(w), ws.cand_n(w), ws.cand_bits(w));
    VN_LAUNCH_STATUS();
    if (stats) {
        k_as_count<SLOTS><<<boxes, SLOTS, 0, st>>>(N, max_gt, ws.best_bits(w), ws.best_arg(w), ws.cand_n(w), ws.cand_bits(w), stats, stride, col);
        VN_LAUNCH_STATUS();
    }
    k_as_encode<AS_ENC_THREADS><<<grid, AS_ENC_THREADS, 0, st>>>(anchors, N, gt, max_gt, ws.best_bits(w), ws.best_arg(w), anchor_h, pos, neg,
                                                                 targets, matched);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

}  // namespace
