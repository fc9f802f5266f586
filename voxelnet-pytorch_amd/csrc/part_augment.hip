// Part-aware object augmentation — the per-point half (SE-SSD's "shape-aware", PA-AUG's "part-aware" augmentation;
// DESIGN.md section 1a-quinquies).  An object's box is cut into the six pyramids that join its centre to its faces; per
// object one pyramid may lose all its points (an occluded side), one may be thinned (a farther, sparser return) and one
// may be exchanged with the same pyramid of another object of its class, rescaled to that object's box.  The O(boxes)
// half — the draw, the pairing, the extent ratios — stays on the host (voxelnet_amd/part_augment.py); this file runs on
// the pipeline's stream between the paste and the augmentation.  The reference has no counterpart.
//
// For a float32 point (px, py, pz) widened exactly to float64 and its owner's entry, in float64 exactly as written (no
// contraction: the Makefile builds with -ffp-contract=off), no divide:
//   owner  : the LOWEST live entry whose box holds the point — vn_gt_inside of common.h, inclusive; a row with a NaN in
//            x, y or z has none.  Entry o is dead when gate != NULL, o >= gate_first and gate[o - gate_first] < gate_min.
//   pyramid: dx = px - x; dy = py - y; u = dx*c + dy*s; v = -(dx*s) + dy*c; hh = (z1 - z0) * 0.5; w = pz - (z0 + hh)
//            m0 = |u| * (hw*hh); m1 = |v| * (hl*hh); m2 = |w| * (hl*hw)      (|coordinate| / half extent, cross-multiplied)
//            axis = 0 when m0 >= m1 and m0 >= m2, else 1 when m1 >= m2, else 2;  f = 2*axis + (coordinate < 0 ? 1 : 0)
//   drop   : bit f of drop_mask -> a NaN point
//   thin   : bit f of sparse_mask, counts[o][f] >= sparse_min, (fmix32(i ^ sparse_key) >> 8) >= sparse_thresh -> a NaN point
//   swap   : bit f of swap_mask, p = swap_with a live entry other than o:
//            X = p.x + (u*ru * p.c - v*rv * p.s); Y = p.y + (u*ru * p.s + v*rv * p.c); Z = (p.z0 + hh_p) + w*rw
//   the first rule that applies wins; every other row is a BIT copy (one 16-byte word).
// Three launches, separated by kernel boundaries only (no workgroup waits on another one):
//   k_part_zero : the 6 counts and 3 stats per entry
//   k_part_count: one thread per row; the boxes' first 64 bytes (<= 8 KB) and the live flags staged once per workgroup in
//                 LDS and read at wave-uniform addresses; the float64 sweep stops at the first hit; owner and pyramid go to
//                 the workspace as one uint16 per row, so the apply pass sweeps nothing; the counts are a per-workgroup
//                 LDS histogram flushed with one global integer add per non-empty bin
//   k_part_apply: one thread per row; an owned row reads its owner's entry (and a swap its partner's) from the table in
//                 global memory — a few percent of a frame's rows are owned, so nothing is staged; the stats are gathered
//                 like the counts.
// Integer adds only: the result does not depend on the order of the atomics.  16 B read + 2 B written per row in the
// count pass, 2 B read per row in the apply pass (+ 16 B read and written per changed — or, out of place, every — row).
#include "common.h"

namespace {

static_assert(sizeof(vnPartBox) == 128 && offsetof(vnPartBox, ru) == sizeof(vnGtBox), "vnPartBox begins with vnGtBox's fields");

constexpr unsigned PART_NONE = 0xFFFFu;          // a row without an owner; an owned row's code is owner * 8 + pyramid
constexpr int PART_FACES = 6, PART_STATS = 3;

__device__ __forceinline__ bool part_dead(const int32_t *__restrict__ gate, int gate_first, int gate_min, int o) {
    return gate != nullptr && o >= gate_first && gate[o - gate_first] < gate_min;
}

// local coordinates of a point in its owner's box and the pyramid that holds it, exactly as the header writes them
template <typename Box>
__device__ __forceinline__ int part_pyramid(double px, double py, double pz, const Box &q, double &u, double &v, double &w) {
    const double dx = px - q.x, dy = py - q.y;
    u = dx * q.c + dy * q.s;
    v = -(dx * q.s) + dy * q.c;
    const double hh = (q.z1 - q.z0) * 0.5;
    w = pz - (q.z0 + hh);
    const double m0 = fabs(u) * (q.hw * hh), m1 = fabs(v) * (q.hl * hh), m2 = fabs(w) * (q.hl * q.hw);
    const int axis = (m0 >= m1 && m0 >= m2) ? 0 : (m1 >= m2 ? 1 : 2);
    const double along = axis == 0 ? u : (axis == 1 ? v : w);
    return 2 * axis + (along < 0.0 ? 1 : 0);
}

__global__ void __launch_bounds__(256) k_part_zero(int32_t *__restrict__ counts, int32_t *__restrict__ stats, int n_boxes) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_boxes * PART_FACES) counts[i] = 0;
    if (i < n_boxes * PART_STATS) stats[i] = 0;
}

__global__ void __launch_bounds__(256) k_part_count(const float4 *__restrict__ pts, uint32_t n, const vnPartBox *__restrict__ boxes,
                                                    int n_boxes, const int32_t *__restrict__ gate, int gate_first, int gate_min,
                                                    uint16_t *__restrict__ code, int32_t *__restrict__ counts) {
    __shared__ __attribute__((aligned(16))) vnGtBox tab[VN_PART_MAX_BOXES];
    __shared__ int hist[VN_PART_MAX_BOXES * PART_FACES];
    __shared__ int live[VN_PART_MAX_BOXES];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(boxes);          // eight words per entry, the box is the first four
        uint4 *dst = reinterpret_cast<uint4 *>(tab);
        for (int w = threadIdx.x; w < n_boxes * 4; w += 256) dst[w] = src[(w >> 2) * 8 + (w & 3)];
        for (int b = threadIdx.x; b < n_boxes * PART_FACES; b += 256) hist[b] = 0;
        if ((int)threadIdx.x < n_boxes) live[threadIdx.x] = part_dead(gate, gate_first, gate_min, threadIdx.x) ? 0 : 1;
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        const float4 p = pts[i];
        unsigned c = PART_NONE;
        if (!(p.x != p.x || p.y != p.y || p.z != p.z)) {
            const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
            for (int b = 0; b < n_boxes; ++b) {
                if (live[b] && vn_gt_inside(px, py, pz, tab[b])) {          // (wave-uniform addresses: LDS broadcasts)
                    double u, v, w;
                    const int f = part_pyramid(px, py, pz, tab[b], u, v, w);
                    c = (unsigned)(b * 8 + f);
                    atomicAdd(&hist[b * PART_FACES + f], 1);
                    break;                                                   // the first hit ends the sweep
                }
            }
        }
        code[i] = (uint16_t)c;
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_boxes * PART_FACES; b += 256)
        if (hist[b]) atomicAdd(&counts[b], hist[b]);
}

// (pts / out carry no __restrict__: out may BE pts — every thread reads its own row, then writes the same row)
__global__ void __launch_bounds__(256) k_part_apply(const uint4 *pts, uint32_t n, const vnPartBox *__restrict__ boxes, int n_boxes,
                                                    const int32_t *__restrict__ gate, int gate_first, int gate_min,
                                                    const uint16_t *__restrict__ code, const int32_t *__restrict__ counts, uint4 *out,
                                                    int32_t *__restrict__ stats, int copy) {
    __shared__ int hist[VN_PART_MAX_BOXES * PART_STATS];
    for (int b = threadIdx.x; b < n_boxes * PART_STATS; b += 256) hist[b] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        const unsigned c = code[i];
        if (c == PART_NONE) {
            if (copy) out[i] = pts[i];
        } else {
            const int o = (int)(c >> 3), f = (int)(c & 7u);                  // written by k_part_count: o < n_boxes, f < 6
            const vnPartBox &q = boxes[o];
            const int bit = 1 << f;
            uint4 r = pts[i];
            int rule = -1;
            if ((q.drop_mask & 0x3F) & bit) {
                rule = 0;
            } else if (((q.sparse_mask & 0x3F) & bit) && counts[o * PART_FACES + f] >= q.sparse_min &&
                       (vn_fmix32(i ^ q.sparse_key) >> 8) >= q.sparse_thresh) {
                rule = 1;
            } else if ((q.swap_mask & 0x3F) & bit) {
                const int p = q.swap_with;
                if ((unsigned)p < (unsigned)n_boxes && p != o && !part_dead(gate, gate_first, gate_min, p)) {
                    const vnPartBox &t = boxes[p];
                    double u, v, w;
                    part_pyramid((double)__uint_as_float(r.x), (double)__uint_as_float(r.y), (double)__uint_as_float(r.z), q, u, v, w);
                    const double u2 = u * q.ru, v2 = v * q.rv, w2 = w * q.rw;
                    const double hh = (t.z1 - t.z0) * 0.5;
                    r.x = __float_as_uint((float)(t.x + (u2 * t.c - v2 * t.s)));
                    r.y = __float_as_uint((float)(t.y + (u2 * t.s + v2 * t.c)));
                    r.z = __float_as_uint((float)((t.z0 + hh) + w2));
                    rule = 2;
                }
            }
            if (rule == 0 || rule == 1) r = make_uint4(0x7FC00000u, 0x7FC00000u, 0x7FC00000u, 0x7FC00000u);
            if (rule >= 0) atomicAdd(&hist[o * PART_STATS + rule], 1);
            if (rule >= 0 || copy) out[i] = r;
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < n_boxes * PART_STATS; b += 256)
        if (hist[b]) atomicAdd(&stats[b], hist[b]);
}

inline bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool bytes_overlap(const void *a, const void *b, size_t bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return bytes > 0 && a0 < b0 + bytes && b0 < a0 + bytes;
}

}  // namespace

extern "C" size_t vn_part_augment_workspace_bytes(int64_t n, int32_t n_boxes) {
    if (n < 0 || n >= (1ll << 31) || n_boxes < 0 || n_boxes > VN_PART_MAX_BOXES) return 0;
    return n_boxes == 0 ? 0 : vn_align((size_t)n * sizeof(uint16_t));          // one (owner, pyramid) code per row
}

extern "C" int vn_part_augment(const float *points, int64_t n, const vnPartBox *boxes, int32_t n_boxes, const int32_t *gate,
                               int32_t gate_first, int32_t gate_min, float *out, int32_t *out_counts, int32_t *out_stats,
                               void *workspace, size_t workspace_bytes, vnStream stream) {
    VN_CHECK_ARG(n >= 0 && n < (1ll << 31));
    VN_CHECK_ARG(n_boxes >= 0 && n_boxes <= VN_PART_MAX_BOXES);
    VN_CHECK_ARG(gate_first >= 0 && gate_first <= n_boxes);
    VN_CHECK_ARG(n == 0 || (points && out));
    VN_CHECK_ARG(n_boxes == 0 || (boxes && out_counts && out_stats));
    const size_t need = vn_part_augment_workspace_bytes(n, n_boxes);
    VN_CHECK_ARG(need == 0 || workspace);
    VN_CHECK_ARG(out == points || !bytes_overlap(out, points, (size_t)n * 16));
    if (workspace_bytes < need) return VN_EWORKSPACE;
    if (n > 0 && (misaligned(points, 16) || misaligned(out, 16))) return VN_EUNSUPPORTED;
    if (n_boxes > 0 && (misaligned(boxes, 16) || misaligned(out_counts, 4) || misaligned(out_stats, 4) || misaligned(gate, 4)))
        return VN_EUNSUPPORTED;
    if (need > 0 && misaligned(workspace, 16)) return VN_EUNSUPPORTED;
    hipStream_t st = vn_stream(stream);
    if (n_boxes == 0) {                                                       // nothing owns anything: a copy
        if (n > 0 && out != points) VN_HIP(hipMemcpyAsync(out, points, (size_t)n * 16, hipMemcpyDeviceToDevice, st));
        return VN_OK;
    }
    k_part_zero<<<(int)vn_ceil_div(n_boxes * PART_FACES, 256), 256, 0, st>>>(out_counts, out_stats, n_boxes);
    VN_LAUNCH_STATUS();
    if (n == 0) return VN_OK;
    const int nb = (int)vn_ceil_div(n, 256);
    uint16_t *code = static_cast<uint16_t *>(workspace);
    k_part_count<<<nb, 256, 0, st>>>(reinterpret_cast<const float4 *>(points), (uint32_t)n, boxes, n_boxes, gate, gate_first, gate_min,
                                     code, out_counts);
    VN_LAUNCH_STATUS();
    k_part_apply<<<nb, 256, 0, st>>>(reinterpret_cast<const uint4 *>(points), (uint32_t)n, boxes, n_boxes, gate, gate_first, gate_min,
                                     code, out_counts, reinterpret_cast<uint4 *>(out), out_stats, out != points ? 1 : 0);
    VN_LAUNCH_STATUS();
    return VN_OK;
}
