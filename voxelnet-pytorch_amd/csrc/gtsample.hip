// Ground-truth database sampling ("GT-paste", SECOND) — the per-point half: which points of a cloud lie inside which
// of up to 128 rotated boxes (vn_points_in_boxes: the database is cut out of the training frames with it), and the
// paste itself (vn_gt_paste: drop the scene points inside the boxes of the objects about to be pasted, keep the rest in
// order, append the objects' points, pad with NaN points).  The O(boxes) half — the draw and the collision test — stays
// on the host (voxelnet_amd/gtsample.py); this file runs on the pipeline's stream between the optional field-of-view
// crop and the augmentation.  The reference has no counterpart.
//
// Inside, for a float32 point (px, py, pz) widened exactly to float64 and a table entry (x, y, z0, z1, hl, hw, c, s):
//   dx = px - x;  dy = py - y;  u = dx*c + dy*s;  v = -(dx*s) + dy*c
//   inside  <=>  |u| <= hl  and  |v| <= hw  and  pz >= z0  and  pz <= z1
// evaluated in float64 exactly as written (no contraction: the Makefile builds with -ffp-contract=off), inclusive; a NaN
// anywhere fails a comparison, so a NaN point is in no box and a box with a NaN field or hl < 0 holds nothing.  c and s
// come from the host.  There is no float32 prefilter: every decision is the float64 one.
// One thread per point, 16-byte loads and stores, the table (<= 8 KB) staged once per workgroup in LDS and read at
// wave-uniform addresses (an LDS broadcast).  The test itself is vn_gt_inside of common.h, shared with augment.hip.
// vn_gt_paste is three launches, the shape of fov.hip: flags + per-workgroup counts (wave ballot + popcount), a
// one-workgroup exclusive scan of the counts, the order-preserving compaction together with the append and the NaN
// fill; the count, scan and rank helpers are the shared ones of common.h.  No workgroup ever waits on another one.
#include "common.h"

namespace {

static_assert(sizeof(vnGtBox) == 64, "vnGtBox is four 16-byte words");

__device__ __forceinline__ void stage_table(vnGtBox *tab, const vnGtBox *__restrict__ boxes, int n_boxes) {
    const uint4 *src = reinterpret_cast<const uint4 *>(boxes);
    uint4 *dst = reinterpret_cast<uint4 *>(tab);
    for (int w = threadIdx.x; w < n_boxes * 4; w += 256) dst[w] = src[w];
}

// COUNTS: every thread walks the whole table (a point inside two boxes counts for both) and the per-box counts are
// gathered by wave ballot -> LDS integer adds -> one global integer add per (workgroup, non-empty box).
template <bool COUNTS>
__global__ void __launch_bounds__(256) k_gt_index(const float4 *__restrict__ pts, int64_t n, const vnGtBox *__restrict__ boxes,
                                                  int n_boxes, int32_t *__restrict__ out_index, int32_t *__restrict__ out_counts) {
    __shared__ __attribute__((aligned(16))) vnGtBox tab[VN_GT_MAX_BOXES];
    __shared__ int cnt[VN_GT_MAX_BOXES];
    stage_table(tab, boxes, n_boxes);
    if (COUNTS && threadIdx.x < VN_GT_MAX_BOXES) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    const float q = __builtin_nanf("");
    const float4 p = live ? pts[i] : make_float4(q, q, q, q);          // (a NaN point is in no box)
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    int first = -1;
    if (COUNTS) {
        for (int b = 0; b < n_boxes; ++b) {                             // uniform trip count: the ballot sees all 64 lanes
            const bool in = vn_gt_inside(px, py, pz, tab[b]);
            if (in && first < 0) first = b;
            const unsigned long long m = __ballot(in);
            if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[b], __popcll(m));
        }
    } else {
        for (int b = 0; b < n_boxes; ++b)
            if (vn_gt_inside(px, py, pz, tab[b])) { first = b; break; }
    }
    if (live) out_index[i] = first;
    if (COUNTS) {
        __syncthreads();
        if ((int)threadIdx.x < n_boxes && cnt[threadIdx.x]) atomicAdd(&out_counts[threadIdx.x], cnt[threadIdx.x]);
    }
}

// launch one of the paste: keep flag per scene row + the number of kept rows per workgroup
__global__ void __launch_bounds__(256) k_gt_flags(const float4 *__restrict__ pts, int64_t n, const vnGtBox *__restrict__ boxes,
                                                  int n_boxes, uint8_t *__restrict__ flags, int32_t *__restrict__ block_counts) {
    __shared__ __attribute__((aligned(16))) vnGtBox tab[VN_GT_MAX_BOXES];
    stage_table(tab, boxes, n_boxes);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < n) {
        const float4 p = pts[i];
        keep = !(p.x != p.x || p.y != p.y || p.z != p.z);              // the padding rows of vn_fov_crop go
        if (keep) {
            const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
            for (int b = 0; b < n_boxes; ++b)
                if (vn_gt_inside(px, py, pz, tab[b])) { keep = false; break; }      // the first hit ends the walk
        }
        flags[i] = keep ? 1 : 0;
    }
    const int kept = vn_block_count(keep);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = kept;
}

// launch two: exclusive scan of the block counts in place (one workgroup; nb may be 0), the number of kept rows -> *kept,
// kept + m -> *count
__global__ void __launch_bounds__(256) k_gt_scan(int32_t *__restrict__ block_counts, int nb, int32_t m, int32_t *__restrict__ kept,
                                                 int32_t *__restrict__ count) {
    const int32_t total = vn_scan_block_sums<int32_t, 256>(block_counts, nb);
    if (threadIdx.x == 0) {
        *kept = total;
        *count = total + m;
    }
}

// launch three, over the cap rows of the output: thread i < n moves scene row i to its place below k when it is kept;
// thread i >= k writes output row i itself — an object row for i < k + m, a NaN point after that.  (Rows below k are
// written by the kept scene rows only, rows from k on by their own thread only.)
__global__ void __launch_bounds__(256) k_gt_compact(const float4 *__restrict__ pts, int64_t n, const uint8_t *__restrict__ flags,
                                                    const int32_t *__restrict__ block_offsets, const float4 *__restrict__ obj,
                                                    int64_t m, float4 *__restrict__ out, int64_t cap,
                                                    const int32_t *__restrict__ kept) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < n && flags[i];
    const int rank = vn_block_rank(keep);
    if (keep) out[block_offsets[blockIdx.x] + rank] = pts[i];
    const int64_t k = (int64_t)kept[0];
    if (i < cap && i >= k) {
        const float q = __builtin_nanf("");
        out[i] = i - k < m ? obj[i - k] : make_float4(q, q, q, q);
    }
}

inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
inline bool ranges_overlap(const void *a, int64_t a_rows, const void *b, int64_t b_rows) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a_rows > 0 && b_rows > 0 && a0 < b0 + (uintptr_t)b_rows * 16 && b0 < a0 + (uintptr_t)a_rows * 16;
}
inline size_t flags_bytes(int64_t n) { return vn_align((size_t)(n > 0 ? n : 1)); }

}  // namespace

extern "C" int vn_points_in_boxes(const float *points, int64_t n, const vnGtBox *boxes, int32_t n_boxes, int32_t *out_index,
                                  int32_t *out_counts, vnStream stream) {
    VN_CHECK_ARG(n >= 0 && n < (1ll << 31) && n_boxes >= 0 && n_boxes <= VN_GT_MAX_BOXES);
    VN_CHECK_ARG(n_boxes == 0 || boxes);
    VN_CHECK_ARG(n == 0 || (points && out_index));
    if ((n > 0 && misaligned(points)) || (n_boxes > 0 && misaligned(boxes))) return VN_EUNSUPPORTED;
    hipStream_t st = vn_stream(stream);
    if (out_counts && n_boxes > 0) VN_HIP(hipMemsetAsync(out_counts, 0, (size_t)n_boxes * sizeof(int32_t), st));
    if (n == 0) return VN_OK;
    const int nb = (int)vn_ceil_div(n, 256);
    const float4 *src = reinterpret_cast<const float4 *>(points);
    if (out_counts && n_boxes > 0)
        k_gt_index<true><<<nb, 256, 0, st>>>(src, n, boxes, n_boxes, out_index, out_counts);
    else
        k_gt_index<false><<<nb, 256, 0, st>>>(src, n, boxes, n_boxes, out_index, nullptr);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" size_t vn_gt_paste_workspace_bytes(int64_t n) {
    if (n < 0 || n >= (1ll << 31)) return 0;
    // flags (n bytes) | per-workgroup counts / offsets (int32 each) | the number of kept scene rows (int32)
    return flags_bytes(n) + vn_align((size_t)(vn_ceil_div(n > 0 ? n : 1, 256) + 1) * sizeof(int32_t));
}

extern "C" int vn_gt_paste(const float *points, int64_t n, const vnGtBox *boxes, int32_t n_boxes, const float *obj_points,
                           int64_t m, float *out_points, int64_t cap, int32_t *out_count, void *workspace,
                           size_t workspace_bytes, vnStream stream) {
    VN_CHECK_ARG(n >= 0 && n < (1ll << 31) && m >= 0 && m < (1ll << 31) && cap >= 0 && cap < (1ll << 31));
    VN_CHECK_ARG(n_boxes >= 0 && n_boxes <= VN_GT_MAX_BOXES && out_count && workspace);
    VN_CHECK_ARG(cap >= n + m);
    VN_CHECK_ARG((n == 0 || points) && (m == 0 || obj_points) && (cap == 0 || out_points) && (n_boxes == 0 || boxes));
    VN_CHECK_ARG(!ranges_overlap(out_points, cap, points, n) && !ranges_overlap(out_points, cap, obj_points, m));
    if (workspace_bytes < vn_gt_paste_workspace_bytes(n)) return VN_EWORKSPACE;
    if ((n > 0 && misaligned(points)) || (m > 0 && misaligned(obj_points)) || (cap > 0 && misaligned(out_points)) ||
        (n_boxes > 0 && misaligned(boxes)))
        return VN_EUNSUPPORTED;
    hipStream_t st = vn_stream(stream);
    uint8_t *flags = static_cast<uint8_t *>(workspace);
    int32_t *counts = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + flags_bytes(n));
    const int nb = (int)vn_ceil_div(n, 256);
    int32_t *kept = counts + (nb > 0 ? nb : 1);
    const float4 *src = reinterpret_cast<const float4 *>(points);
    if (n > 0) {
        k_gt_flags<<<nb, 256, 0, st>>>(src, n, boxes, n_boxes, flags, counts);
        VN_LAUNCH_STATUS();
    }
    k_gt_scan<<<1, 256, 0, st>>>(counts, nb, (int32_t)m, kept, out_count);
    VN_LAUNCH_STATUS();
    if (cap > 0) {
        k_gt_compact<<<(int)vn_ceil_div(cap, 256), 256, 0, st>>>(src, n, flags, counts, reinterpret_cast<const float4 *>(obj_points),
                                                                m, reinterpret_cast<float4 *>(out_points), cap, kept);
        VN_LAUNCH_STATUS();
    }
    return VN_OK;
}
