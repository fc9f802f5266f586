// SECOND's anchor mask (anchor_area_threshold): an anchor over whose bird's-eye footprint the frame
// has (almost) no occupied voxel takes no part in the loss and can never become a detection.  Integer work throughout —
// every output is held to exact equality with a brute-force restatement (tests/anchor_mask_ref.py).
//
// Definitions (include/voxelnet_hip.h states them in full).  coord (K,4) int64 rows [b, d, h, w];
//   occ[b,h,w]  = the number of rows of coord with that (b, h, w): rows are counted, not de-duplicated, and a row with b
//                 outside [0,B), h outside [0,H) or w outside [0,W) is ignored — neither counted nor written anywhere;
//   rects (N,4) = [w0, h0, w1, h1] int32, the INCLUSIVE cell rectangle of every anchor in anchor order n = 2 * site + a
//                 (host work, voxelnet_amd/anchor_mask.py anchor_cell_rects); w1 < w0 or h1 < h0: empty, count 0;
//   count[b,n]  = sum of occ[b, h0..h1, w0..w1] — the whole rectangle, its first row and column included;
//   mask[b,n]   = count[b,n] > threshold.
//
// Launches of vn_anchor_mask: one memset (the table S), then
//   k_am_count  one thread per row of coord: an int32 atomicAdd on S[b, h+1, w+1].  Integer atomics of an order-free sum:
//               bit-identical from run to run; there is no floating-point atomic anywhere.
//   k_am_rows   S is the summed-area table (B, H+1, W+1) int32 with a zero first row and column, built in place.  Row pass:
//               one workgroup per (b, h), common.h's vn_block_excl_scan over chunks of AM_THREADS cells with a carry.
//   k_am_segs   column pass, first half: the rows 1..H are cut into segments of AM_SEG; one thread per (b, segment, w)
//               sums its segment's AM_SEG values — coalesced across w, the loads independent of the sum (all in flight).
//   k_am_cols   second half: one thread per (b, segment, w) adds the totals of the segments above (ceil(H / AM_SEG) - 1
//               independent loads at most) and walks its own AM_SEG rows, loaded ahead of the running sum, in place.
//               No thread walks the whole height.
//   k_am_query  one thread per (b, n): four reads of S, mask and (optional) count; with pos / neg given, 0.0f is stored
//               where the anchor is masked out — a kept anchor's two floats are not written at all.
// vn_anchor_mask_probs: k_am_probs, elementwise, a masked-out anchor's score is +0.0f in a COPY of the probability map.
#include "common.h"

namespace {

constexpr int AM_THREADS = 256;          // workgroup size; the row scan's chunk
constexpr int AM_SEG = 32;               // rows per column segment

__global__ void __launch_bounds__(AM_THREADS) k_am_count(const int64_t *__restrict__ coord, int64_t K, int B, int H, int W,
                                                         int32_t *__restrict__ S) {
    const int64_t i = (int64_t)blockIdx.x * AM_THREADS + threadIdx.x;
    if (i >= K) return;
    const int64_t b = coord[i * 4], h = coord[i * 4 + 2], w = coord[i * 4 + 3];
    if (b < 0 || b >= B || h < 0 || h >= H || w < 0 || w >= W) return;
    atomicAdd(S + ((size_t)b * (H + 1) + (size_t)h + 1) * (W + 1) + (size_t)w + 1, 1);
}

// row (b, h + 1) of S: cell w + 1 becomes occ[b, h, 0..w] summed; column 0 stays the memset's zero
__global__ void __launch_bounds__(AM_THREADS) k_am_rows(int32_t *__restrict__ S, int H, int W) {
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    int32_t *row = S + ((size_t)b * (H + 1) + (size_t)h + 1) * (W + 1) + 1;
    int32_t carry = 0;
    for (int base = 0; base < W; base += AM_THREADS) {
        const int w = base + threadIdx.x;
        const int32_t v = w < W ? row[w] : 0;
        int32_t tot;
        const int32_t ex = vn_block_excl_scan<int32_t, AM_THREADS>(v, &tot);
        if (w < W) row[w] = carry + ex + v;
        carry += tot;
    }
}

// which (b, segment, column) a thread of the two column kernels works on; false past the last column
__device__ __forceinline__ bool am_seg_of(int H, int W, int &b, int &s, int &w) {
    const int nseg = (H + AM_SEG - 1) / AM_SEG, wt = (W + AM_THREADS) / AM_THREADS;          // (W + 1 columns)
    int id = blockIdx.x;
    w = (id % wt) * AM_THREADS + threadIdx.x; id /= wt;
    s = id % nseg;
    b = id / nseg;
    return w <= W;
}

__global__ void __launch_bounds__(AM_THREADS) k_am_segs(const int32_t *__restrict__ S, int H, int W, int32_t *__restrict__ tot) {
    int b, s, w;
    if (!am_seg_of(H, W, b, s, w)) return;
    const int nseg = (H + AM_SEG - 1) / AM_SEG;
    const int r0 = 1 + s * AM_SEG;
    const int32_t *col = S + ((size_t)b * (H + 1) + r0) * (W + 1) + w;
    int32_t v[AM_SEG];
#pragma unroll
    for (int j = 0; j < AM_SEG; ++j) v[j] = r0 + j <= H ? col[(size_t)j * (W + 1)] : 0;
    int32_t sum = 0;
#pragma unroll
    for (int j = 0; j < AM_SEG; ++j) sum += v[j];
    tot[((size_t)b * nseg + s) * (W + 1) + w] = sum;
}

__global__ void __launch_bounds__(AM_THREADS) k_am_cols(int32_t *__restrict__ S, int H, int W, const int32_t *__restrict__ tot) {
    int b, s, w;
    if (!am_seg_of(H, W, b, s, w)) return;
    const int nseg = (H + AM_SEG - 1) / AM_SEG;
    const int r0 = 1 + s * AM_SEG;
    int32_t *col = S + ((size_t)b * (H + 1) + r0) * (W + 1) + w;
    int32_t v[AM_SEG];
#pragma unroll
    for (int j = 0; j < AM_SEG; ++j) v[j] = r0 + j <= H ? col[(size_t)j * (W + 1)] : 0;
    int32_t run = 0;
    const int32_t *t = tot + (size_t)b * nseg * (W + 1) + w;
    for (int q = 0; q < s; ++q) run += t[(size_t)q * (W + 1)];
#pragma unroll
    for (int j = 0; j < AM_SEG; ++j) {
        run += v[j];
        if (r0 + j <= H) col[(size_t)j * (W + 1)] = run;
    }
}

__global__ void __launch_bounds__(AM_THREADS) k_am_query(const int32_t *__restrict__ S, int H, int W, const int4 *__restrict__ rects,
                                                         int N, int64_t total, int threshold, uint8_t *__restrict__ mask,
                                                         int32_t *__restrict__ count, float *__restrict__ pos, float *__restrict__ neg) {
    const int64_t o = (int64_t)blockIdx.x * AM_THREADS + threadIdx.x;
    if (o >= total) return;
    const int b = (int)(o / N), n = (int)(o % N);
    const int4 r = rects[n];
    // (a table from anchor_cell_rects is clipped already; the clamp keeps a foreign one inside S)
    const int w0 = max(r.x, 0), h0 = max(r.y, 0), w1 = min(r.z, W - 1), h1 = min(r.w, H - 1);
    int32_t c = 0;
    if (w1 >= w0 && h1 >= h0) {
        const int32_t *Sb = S + (size_t)b * (H + 1) * (W + 1);
        const size_t top = (size_t)h0 * (W + 1), bot = (size_t)(h1 + 1) * (W + 1);
        c = Sb[bot + w1 + 1] - Sb[top + w1 + 1] - Sb[bot + w0] + Sb[top + w0];
    }
    const bool keep = c > threshold;
    mask[o] = keep ? 1 : 0;
    if (count) count[o] = c;
    if (pos && !keep) {
        pos[o] = 0.0f;
        neg[o] = 0.0f;
    }
}

template <int LAYOUT>
__global__ void __launch_bounds__(AM_THREADS) k_am_probs(const float *__restrict__ probs, const uint8_t *__restrict__ mask, int N,
                                                         int64_t total, float *__restrict__ out) {
    const int64_t o = (int64_t)blockIdx.x * AM_THREADS + threadIdx.x;
    if (o >= total) return;
    int64_t m = o;          // VN_DETECT_FLAT: flat element e of probs[b] is anchor e
    if (LAYOUT == VN_DETECT_SITE) {          // element a * S + s of probs[b] is anchor 2 * s + a
        const int64_t b = o / N;
        const int e = (int)(o % N), sites = N / 2;
        m = b * N + 2 * (int64_t)(e % sites) + e / sites;
    }
    out[o] = mask[m] ? probs[o] : 0.0f;
}

inline bool am_args_ok(int32_t B, int32_t H, int32_t W, int32_t N) {
    return B > 0 && H > 0 && W > 0 && N > 0 && (int64_t)B * ((int64_t)H + 1) * ((int64_t)W + 1) < (1ll << 28) &&
           (int64_t)B * N < (1ll << 28);
}
inline int am_nseg(int32_t H) { return (H + AM_SEG - 1) / AM_SEG; }
inline size_t am_table_bytes(int32_t B, int32_t H, int32_t W) {
    return vn_align((size_t)B * ((size_t)H + 1) * ((size_t)W + 1) * sizeof(int32_t));
}
inline size_t am_tot_bytes(int32_t B, int32_t H, int32_t W) {
    return vn_align((size_t)B * am_nseg(H) * ((size_t)W + 1) * sizeof(int32_t));
}

}  // namespace

// workspace: [S (B, H+1, W+1) | segment totals (B, ceil(H / AM_SEG), W+1)]; S is cleared by the call, the totals are
// written in full before they are read
extern "C" size_t vn_anchor_mask_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t n_anchors) {
    if (!am_args_ok(B, H, W, n_anchors)) return 0;
    return am_table_bytes(B, H, W) + am_tot_bytes(B, H, W);
}

extern "C" int vn_anchor_mask(const int64_t *coord, int64_t K, int32_t B, int32_t H, int32_t W, const int32_t *rects,
                              int32_t n_anchors, int32_t threshold, uint8_t *mask, int32_t *count, float *pos, float *neg,
                              void *workspace, size_t workspace_bytes, vnStream stream) {
    VN_CHECK_ARG(am_args_ok(B, H, W, n_anchors) && K >= 0 && K < (1ll << 31) && (coord || K == 0) && rects && mask && workspace);
    VN_CHECK_ARG(threshold >= 0 && (pos != nullptr) == (neg != nullptr));
    if (reinterpret_cast<uintptr_t>(rects) % 16 || reinterpret_cast<uintptr_t>(workspace) % 4) return VN_EUNSUPPORTED;
    if (workspace_bytes < vn_anchor_mask_workspace_bytes(B, H, W, n_anchors)) return VN_EWORKSPACE;
    hipStream_t st = vn_stream(stream);
    int32_t *S = static_cast<int32_t *>(workspace);
    int32_t *tot = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + am_table_bytes(B, H, W));
    VN_HIP(hipMemsetAsync(S, 0, am_table_bytes(B, H, W), st));
    if (K > 0) {          // (K == 0: S is all zero already, every count is 0)
        k_am_count<<<(unsigned)vn_ceil_div(K, AM_THREADS), AM_THREADS, 0, st>>>(coord, K, B, H, W, S);
        VN_LAUNCH_STATUS();
        k_am_rows<<<(unsigned)(B * H), AM_THREADS, 0, st>>>(S, H, W);
        VN_LAUNCH_STATUS();
        const unsigned blocks = (unsigned)((int64_t)B * am_nseg(H) * ((W + AM_THREADS) / AM_THREADS));
        k_am_segs<<<blocks, AM_THREADS, 0, st>>>(S, H, W, tot);
        VN_LAUNCH_STATUS();
        k_am_cols<<<blocks, AM_THREADS, 0, st>>>(S, H, W, tot);
        VN_LAUNCH_STATUS();
    }
    const int64_t total = (int64_t)B * n_anchors;
    k_am_query<<<(unsigned)vn_ceil_div(total, AM_THREADS), AM_THREADS, 0, st>>>(S, H, W, reinterpret_cast<const int4 *>(rects),
                                                                                 n_anchors, total, threshold, mask, count, pos, neg);
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" int vn_anchor_mask_probs(const float *probs, const uint8_t *mask, int32_t B, int32_t n_anchors, int32_t layout,
                                    float *out, vnStream stream) {
    VN_CHECK_ARG(probs && mask && out && B > 0 && n_anchors > 0 && (int64_t)B * n_anchors < (1ll << 28));
    VN_CHECK_ARG(layout == VN_DETECT_FLAT || (layout == VN_DETECT_SITE && n_anchors % 2 == 0));
    const int64_t total = (int64_t)B * n_anchors;
    const char *p = reinterpret_cast<const char *>(probs), *o = reinterpret_cast<const char *>(out);
    VN_CHECK_ARG(o + total * sizeof(float) <= p || p + total * sizeof(float) <= o);          // out may not alias probs
    hipStream_t st = vn_stream(stream);
    const unsigned blocks = (unsigned)vn_ceil_div(total, AM_THREADS);
    if (layout == VN_DETECT_FLAT)
        k_am_probs<VN_DETECT_FLAT><<<blocks, AM_THREADS, 0, st>>>(probs, mask, n_anchors, total, out);
    else
        k_am_probs<VN_DETECT_SITE><<<blocks, AM_THREADS, 0, st>>>(probs, mask, n_anchors, total, out);
    VN_LAUNCH_STATUS();
    return VN_OK;
}
