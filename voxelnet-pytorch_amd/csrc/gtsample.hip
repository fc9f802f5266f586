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
//
// vn_gt_paste_visible is the occlusion-consistent paste: a coarse range image of the frame
// — four side faces of a cube around the sensor, nu x nv bins each, depth = max(|x|, |y|), all float64 as written —
// rejects pasted objects that hide behind scene points, drops the hidden points of the others and the scene (and other
// objects') points in their shadow.  Seven launches, separated by kernel boundaries only: reset of the two depth buffers
// and the counters, scene depth (atomicMin on the float's bit pattern), visible points per object (ballot + popcount ->
// LDS adds -> one global add per workgroup and object), object depth with its owner (64-bit atomicMin of depth << 32 |
// object), keep flags over the concatenated n + m rows + per-workgroup counts, the shared one-workgroup scan
// (k_gt_scan), compaction + NaN fill.  Minima and integer sums do not depend on the order of the atomics.
#include <cmath>
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

// ---- vn_gt_paste_visible ------------------------------------------------------------------------------------------------
// the objects' row offsets (n_boxes + 1 values, read and validated on the host at call time), passed to the kernels by
// value and staged in LDS once per workgroup
struct VisOffsets {
    int32_t v[VN_GT_MAX_BOXES + 1];
};
constexpr unsigned VIS_EMPTY32 = 0xFFFFFFFFu;
constexpr unsigned long long VIS_EMPTY64 = ~0ull;

__device__ __forceinline__ void stage_offsets(int *off, const VisOffsets &offs, int n_boxes) {
    if ((int)threadIdx.x <= n_boxes) off[threadIdx.x] = offs.v[threadIdx.x];
}

// bin and depth of a point, float64 exactly as the header writes it; false = no bin.  0 <= bin < 4 * nv * nu.
__device__ __forceinline__ bool vis_bin(const float4 &p, const vnVisGrid &g, int &bin, unsigned &depth) {
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    const double ax = fabs(px), ay = fabs(py);
    double a, u;
    int face;
    if (ax >= ay) {
        a = ax;
        face = px > 0.0 ? 0 : 2;
        u = py / a;
    } else {
        a = ay;
        face = py > 0.0 ? 1 : 3;
        u = px / a;
    }
    const double v = pz / a;
    if (!(isfinite(px) && isfinite(py) && isfinite(pz)) || a == 0.0) return false;
    const double fu = fmin(floor((u + 1.0) * (double)(g.nu / 2)), (double)(g.nu - 1));
    const double fv = floor((v - g.v_lo) * g.v_scale);
    if (!(fv >= 0.0 && fv < (double)g.nv)) return false;
    bin = (face * g.nv + (int)fv) * g.nu + (int)fu;
    depth = __float_as_uint((float)a);          // a is |x| or |y| of a float32 point: exact, and its bits order like it
    return true;
}
__device__ __forceinline__ bool vis_behind(unsigned depth, unsigned front, double margin) {
    return (double)__uint_as_float(depth) > (double)__uint_as_float(front) + margin;
}
__device__ __forceinline__ bool vis_nan(const float4 &p) { return p.x != p.x || p.y != p.y || p.z != p.z; }

// the object that owns object row j: the largest o with off[o] <= j (0 <= j < off[n_boxes]; empty objects own nothing)
__device__ __forceinline__ int vis_owner(const int *off, int n_boxes, int j) {
    int lo = 0, hi = n_boxes;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}
// per-object count of a flag over the workgroup's object rows, the scheme of k_gt_index<counts>: objects o_lo..o_hi are
// the workgroup's (uniform trip count, so each ballot sees all 64 lanes)
__device__ __forceinline__ void vis_count_objects(int *cnt, bool flag, int o, int o_lo, int o_hi) {
    for (int b = o_lo; b <= o_hi; ++b) {
        const unsigned long long mk = __ballot(flag && o == b);
        if ((threadIdx.x & 63) == 0 && mk) atomicAdd(&cnt[b], __popcll(mk));
    }
}

// launch one: both depth buffers (one contiguous run of 16-byte words) to "empty", the counters to 0
__global__ void __launch_bounds__(256) k_vis_reset(uint4 *__restrict__ depth, int64_t words, int32_t *__restrict__ visible,
                                                   int32_t *__restrict__ kept, int n_boxes, int32_t *__restrict__ stats) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < words) depth[i] = make_uint4(VIS_EMPTY32, VIS_EMPTY32, VIS_EMPTY32, VIS_EMPTY32);
    if (blockIdx.x == 0) {
        if ((int)threadIdx.x < n_boxes) {
            visible[threadIdx.x] = 0;
            kept[threadIdx.x] = 0;
        }
        if (threadIdx.x < 2) stats[threadIdx.x] = 0;
    }
}

// launch two: Dscene[bin] = the nearest scene row that has a bin and lies inside no box of the table
__global__ void __launch_bounds__(256) k_vis_scene_depth(const float4 *__restrict__ pts, int64_t n, const vnGtBox *__restrict__ boxes,
                                                         int n_boxes, vnVisGrid g, unsigned *__restrict__ dscene) {
    __shared__ __attribute__((aligned(16))) vnGtBox tab[VN_GT_MAX_BOXES];
    stage_table(tab, boxes, n_boxes);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    int bin;
    unsigned depth;
    if (!vis_bin(p, g, bin, depth)) return;                             // (a NaN row has no bin)
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    for (int b = 0; b < n_boxes; ++b)
        if (vn_gt_inside(px, py, pz, tab[b])) return;
    atomicMin(&dscene[bin], depth);
}

// launch three: visible flag per object row (kept in the flags of the concatenated rows) + visible[o]
__global__ void __launch_bounds__(256) k_vis_obj_visible(const float4 *__restrict__ obj, int m, VisOffsets offs, int n_boxes,
                                                         vnVisGrid g, const unsigned *__restrict__ dscene,
                                                         uint8_t *__restrict__ obj_flags, int32_t *__restrict__ visible) {
    __shared__ int off[VN_GT_MAX_BOXES + 1];
    __shared__ int cnt[VN_GT_MAX_BOXES];
    stage_offsets(off, offs, n_boxes);
    if (threadIdx.x < VN_GT_MAX_BOXES) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int first = (int)blockIdx.x * 256, last = min(first + 255, m - 1);
    const int j = first + (int)threadIdx.x;
    const int o_lo = vis_owner(off, n_boxes, first), o_hi = vis_owner(off, n_boxes, last);
    bool vis = false;
    int o = -1;
    if (j < m) {
        const float4 p = obj[j];
        o = vis_owner(off, n_boxes, j);
        vis = !vis_nan(p);
        int bin;
        unsigned depth;
        if (vis && vis_bin(p, g, bin, depth)) {
            const unsigned front = dscene[bin];
            if (front != VIS_EMPTY32 && vis_behind(depth, front, g.margin)) vis = false;
        }
        obj_flags[j] = vis ? 1 : 0;
    }
    vis_count_objects(cnt, vis, o, o_lo, o_hi);
    __syncthreads();
    if ((int)threadIdx.x < n_boxes && cnt[threadIdx.x]) atomicAdd(&visible[threadIdx.x], cnt[threadIdx.x]);
}

// launch four: Dobj[bin] = min over the visible points of accepted objects of (depth bits << 32 | object): the nearest
// depth and its owner, equal depths to the lower object
__global__ void __launch_bounds__(256) k_vis_obj_depth(const float4 *__restrict__ obj, int m, VisOffsets offs, int n_boxes, vnVisGrid g,
                                                       const uint8_t *__restrict__ obj_flags, const int32_t *__restrict__ visible,
                                                       unsigned long long *__restrict__ dobj) {
    __shared__ int off[VN_GT_MAX_BOXES + 1];
    stage_offsets(off, offs, n_boxes);
    __syncthreads();
    const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= m || !obj_flags[j]) return;
    const int o = vis_owner(off, n_boxes, j);
    if (visible[o] < g.min_visible) return;
    int bin;
    unsigned depth;
    if (!vis_bin(obj[j], g, bin, depth)) return;
    atomicMin(&dobj[bin], ((unsigned long long)depth << 32) | (unsigned)o);
}

// launch five, over the concatenated n + m rows: the keep flags, the number of kept rows per workgroup, kept[o], stats
__global__ void __launch_bounds__(256) k_vis_flags(const float4 *__restrict__ pts, int n, const vnGtBox *__restrict__ boxes, int n_boxes,
                                                   const float4 *__restrict__ obj, int m, VisOffsets offs, vnVisGrid g,
                                                   const unsigned long long *__restrict__ dobj, const int32_t *__restrict__ visible,
                                                   uint8_t *__restrict__ flags, int32_t *__restrict__ block_counts,
                                                   int32_t *__restrict__ kept, int32_t *__restrict__ stats) {
    __shared__ __attribute__((aligned(16))) vnGtBox tab[VN_GT_MAX_BOXES];
    __shared__ int off[VN_GT_MAX_BOXES + 1];
    __shared__ int cnt[VN_GT_MAX_BOXES];
    __shared__ int accepted[VN_GT_MAX_BOXES];
    __shared__ int st[2];
    stage_table(tab, boxes, n_boxes);
    stage_offsets(off, offs, n_boxes);
    if (threadIdx.x < VN_GT_MAX_BOXES) {
        cnt[threadIdx.x] = 0;
        accepted[threadIdx.x] = (int)threadIdx.x < n_boxes && visible[threadIdx.x] >= g.min_visible;
    }
    if (threadIdx.x < 2) st[threadIdx.x] = 0;
    __syncthreads();
    const int total = n + m;
    const int first = (int)blockIdx.x * 256, last = min(first + 255, total - 1);
    const int i = first + (int)threadIdx.x;
    int o_lo = 0, o_hi = -1;                                            // the workgroup's objects, if it has object rows
    if (last >= n) {
        o_lo = vis_owner(off, n_boxes, max(first, n) - n);
        o_hi = vis_owner(off, n_boxes, last - n);
    }
    bool keep = false, boxed = false, shadowed = false;
    int o = -1;
    if (i < n) {
        const float4 p = pts[i];
        if (!vis_nan(p)) {
            const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
            for (int b = 0; b < n_boxes; ++b)
                if (accepted[b] && vn_gt_inside(px, py, pz, tab[b])) { boxed = true; break; }
            int bin;
            unsigned depth;
            if (!boxed && vis_bin(p, g, bin, depth)) {
                const unsigned long long key = dobj[bin];
                shadowed = key != VIS_EMPTY64 && vis_behind(depth, (unsigned)(key >> 32), g.margin);
            }
            keep = !boxed && !shadowed;
        }
    } else if (i < total) {
        const int j = i - n;
        o = vis_owner(off, n_boxes, j);
        if (flags[i] && accepted[o]) {                                  // visible, of an accepted object
            keep = true;
            int bin;
            unsigned depth;
            if (vis_bin(obj[j], g, bin, depth)) {
                const unsigned long long key = dobj[bin];               // (not empty: this point is a candidate of the bin)
                if ((int)(unsigned)key != o && vis_behind(depth, (unsigned)(key >> 32), g.margin)) keep = false;
            }
        }
    }
    if (i < total) flags[i] = keep ? 1 : 0;
    vis_count_objects(cnt, keep, o, o_lo, o_hi);                        // (o = -1 on scene rows: they match no object)
    const unsigned long long mb = __ballot(boxed), ms = __ballot(shadowed);
    if ((threadIdx.x & 63) == 0) {
        if (mb) atomicAdd(&st[0], __popcll(mb));
        if (ms) atomicAdd(&st[1], __popcll(ms));
    }
    const int n_kept = vn_block_count(keep);                            // (its barrier also completes cnt and st)
    if (threadIdx.x == 0) block_counts[blockIdx.x] = n_kept;
    if ((int)threadIdx.x < n_boxes && cnt[threadIdx.x]) atomicAdd(&kept[threadIdx.x], cnt[threadIdx.x]);
    if (threadIdx.x < 2 && st[threadIdx.x]) atomicAdd(&stats[threadIdx.x], st[threadIdx.x]);
}

// launch seven (six is k_gt_scan with m = 0), over the cap rows of the output: thread i < n + m moves its row — scene
// or object — to its place below the total when it is kept; thread i >= total writes a NaN point to row i itself
__global__ void __launch_bounds__(256) k_vis_compact(const float4 *__restrict__ pts, int n, const float4 *__restrict__ obj, int m,
                                                     const uint8_t *__restrict__ flags, const int32_t *__restrict__ block_offsets,
                                                     float4 *__restrict__ out, int64_t cap, const int32_t *__restrict__ kept_total) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < (int64_t)n + m && flags[i];
    const int rank = vn_block_rank(keep);
    if (keep) out[block_offsets[blockIdx.x] + rank] = i < n ? pts[i] : obj[i - n];
    const int64_t k = (int64_t)kept_total[0];
    if (i < cap && i >= k) {
        const float q = __builtin_nanf("");
        out[i] = make_float4(q, q, q, q);
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

namespace {

inline bool vis_grid_ok(const vnVisGrid *g) {
    return g && g->nu >= 2 && g->nu <= 2048 && g->nu % 2 == 0 && g->nv >= 1 && g->nv <= 256 && std::isfinite(g->v_lo) &&
           std::isfinite(g->v_hi) && g->v_lo < g->v_hi && std::isfinite(g->v_scale) && g->v_scale > 0.0 && g->margin >= 0.0 &&
           g->min_visible >= 0;                                         // (a NaN margin fails margin >= 0; +inf passes)
}
inline int64_t vis_bins(const vnVisGrid *g) { return 4ll * g->nv * g->nu; }          // a multiple of 8
// Dobj (8 bytes per bin) and Dscene (4 bytes per bin) back to back: a whole number of 16-byte words
inline size_t vis_depth_bytes(const vnVisGrid *g) { return (size_t)vis_bins(g) * 12; }

}  // namespace

extern "C" size_t vn_gt_paste_visible_workspace_bytes(int64_t n, int64_t m, const vnVisGrid *grid) {
    if (n < 0 || m < 0 || n + m >= (1ll << 31) || !vis_grid_ok(grid)) return 0;
    // depth buffers | flags (n + m bytes) | per-workgroup counts / offsets (int32 each) | the number of kept rows (int32)
    return vn_align(vis_depth_bytes(grid)) + flags_bytes(n + m) +
           vn_align((size_t)(vn_ceil_div(n + m > 0 ? n + m : 1, 256) + 1) * sizeof(int32_t));
}

extern "C" int vn_gt_paste_visible(const float *points, int64_t n, const vnGtBox *boxes, int32_t n_boxes, const float *obj_points,
                                   int64_t m, const int32_t *obj_offsets, const vnVisGrid *grid, float *out_points, int64_t cap,
                                   int32_t *out_count, int32_t *out_visible, int32_t *out_kept, int32_t *out_stats, void *workspace,
                                   size_t workspace_bytes, vnStream stream) {
    VN_CHECK_ARG(n >= 0 && n < (1ll << 31) && m >= 0 && m < (1ll << 31) && n + m < (1ll << 31) && cap >= 0 && cap < (1ll << 31));
    VN_CHECK_ARG(n_boxes >= 0 && n_boxes <= VN_GT_MAX_BOXES && out_count && out_stats && workspace && obj_offsets);
    VN_CHECK_ARG(vis_grid_ok(grid));
    VN_CHECK_ARG(cap >= n + m);
    VN_CHECK_ARG((n == 0 || points) && (m == 0 || obj_points) && (cap == 0 || out_points) && (n_boxes == 0 || boxes));
    VN_CHECK_ARG(n_boxes == 0 || (out_visible && out_kept));
    VisOffsets offs = {};
    for (int o = 0; o <= n_boxes; ++o) offs.v[o] = obj_offsets[o];
    VN_CHECK_ARG(offs.v[0] == 0 && (int64_t)offs.v[n_boxes] == m);
    for (int o = 0; o < n_boxes; ++o) VN_CHECK_ARG(offs.v[o] <= offs.v[o + 1]);
    VN_CHECK_ARG(!ranges_overlap(out_points, cap, points, n) && !ranges_overlap(out_points, cap, obj_points, m));
    if (workspace_bytes < vn_gt_paste_visible_workspace_bytes(n, m, grid)) return VN_EWORKSPACE;
    if ((n > 0 && misaligned(points)) || (m > 0 && misaligned(obj_points)) || (cap > 0 && misaligned(out_points)) ||
        (n_boxes > 0 && misaligned(boxes)) || misaligned(workspace))
        return VN_EUNSUPPORTED;
    if (((reinterpret_cast<uintptr_t>(out_count) | reinterpret_cast<uintptr_t>(out_stats) | reinterpret_cast<uintptr_t>(out_visible) |
          reinterpret_cast<uintptr_t>(out_kept)) & 3) != 0)
        return VN_EUNSUPPORTED;
    hipStream_t st = vn_stream(stream);
    const vnVisGrid g = *grid;
    const int64_t bins = vis_bins(grid);
    char *ws = static_cast<char *>(workspace);
    unsigned long long *dobj = reinterpret_cast<unsigned long long *>(ws);
    unsigned *dscene = reinterpret_cast<unsigned *>(ws + (size_t)bins * 8);
    uint8_t *flags = reinterpret_cast<uint8_t *>(ws + vn_align(vis_depth_bytes(grid)));
    int32_t *counts = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(flags) + flags_bytes(n + m));
    const int nb = (int)vn_ceil_div(n + m, 256);
    int32_t *kept_total = counts + (nb > 0 ? nb : 1);
    const float4 *src = reinterpret_cast<const float4 *>(points);
    const float4 *obj = reinterpret_cast<const float4 *>(obj_points);
    const int64_t words = (int64_t)(vis_depth_bytes(grid) / 16);
    k_vis_reset<<<(int)vn_ceil_div(words, 256), 256, 0, st>>>(reinterpret_cast<uint4 *>(ws), words, out_visible, out_kept, n_boxes, out_stats);
    VN_LAUNCH_STATUS();
    if (n > 0 && m > 0) {                                               // (without objects nobody reads Dscene)
        k_vis_scene_depth<<<(int)vn_ceil_div(n, 256), 256, 0, st>>>(src, n, boxes, n_boxes, g, dscene);
        VN_LAUNCH_STATUS();
    }
    if (m > 0) {
        const int mb = (int)vn_ceil_div(m, 256);
        k_vis_obj_visible<<<mb, 256, 0, st>>>(obj, (int)m, offs, n_boxes, g, dscene, flags + n, out_visible);
        VN_LAUNCH_STATUS();
        k_vis_obj_depth<<<mb, 256, 0, st>>>(obj, (int)m, offs, n_boxes, g, flags + n, out_visible, dobj);
        VN_LAUNCH_STATUS();
    }
    if (nb > 0) {
        k_vis_flags<<<nb, 256, 0, st>>>(src, (int)n, boxes, n_boxes, obj, (int)m, offs, g, dobj, out_visible, flags, counts, out_kept,
                                        out_stats);
        VN_LAUNCH_STATUS();
    }
    k_gt_scan<<<1, 256, 0, st>>>(counts, nb, 0, kept_total, out_count);
    VN_LAUNCH_STATUS();
    if (cap > 0) {
        k_vis_compact<<<(int)vn_ceil_div(cap, 256), 256, 0, st>>>(src, (int)n, obj, (int)m, flags, counts, reinterpret_cast<float4 *>(out_points),
                                                                 cap, kept_total);
        VN_LAUNCH_STATUS();
    }
    return VN_OK;
}
