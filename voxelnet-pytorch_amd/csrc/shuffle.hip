// The per-sample point shuffle of the input pipeline — the reference's `np.random.shuffle(point_cloud)` in front of the
// voxelizer (voxelnet/utils.py:35), which only decides WHICH <= T points of a crowded voxel survive.  Two forms, both a
// row gather right behind the host->device copy, in front of the crop, the paste and the augmentation:
//   vn_permute_points: out[i] = points[index[i]] — the host draws the index table (np.random.shuffle of arange(n): the
//                      same Mersenne-Twister draws as the shuffle of the cloud itself, so the result is the reference's
//                      bit for bit) and the device moves the rows; an index outside [0, n) gives a NaN point and reads
//                      nothing, so no table can make the kernel read outside `points`
//   vn_shuffle_points: out[i] = points[p(i)], p a keyed bijection of [0, n) evaluated per thread — no host work
//                      proportional to n.  A six-round Feistel network over 2h bits (2^2h < 4n), walked until it lands
//                      inside the range ("cycle walking": F is a bijection of [0, 2^2h), so the walk from i < n comes back
//                      to i at the latest and therefore ends; the values of [0, n) it passes through are skipped by nobody
//                      else, which makes p a bijection).  Exact uint32 arithmetic:
//     k = max(2, bit_length(n - 1));  h = (k + 1) / 2;  mask = 2^h - 1
//     fmix32(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
//     F(x): L = x >> h; R = x & mask; for r in 0..5: (L, R) = (R, L ^ (fmix32(R ^ keys[r]) & mask)); (L << h) | R
//     p(i): x = F(i); while x >= n: x = F(x)
// A row moves as ONE 16-byte integer load and store: NaN payloads, -0.0 and the reflectance survive as bits.
// One thread per output row, 256 threads per workgroup, no LDS, no workspace; no workgroup waits on another one.
// Memory-bound by construction: 16 B read (at a random row) + 16 B written per point, + 4 B of table in the index form.
#include "common.h"

namespace {

struct ShuffleKeys {
    uint32_t k[6];
};

__device__ __forceinline__ uint32_t feistel(uint32_t x, const ShuffleKeys &keys, int h, uint32_t mask) {
    uint32_t L = x >> h, R = x & mask;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const uint32_t t = L ^ (vn_fmix32(R ^ keys.k[r]) & mask);          // (common.h)
        L = R;
        R = t;
    }
    return (L << h) | R;
}

// (n < 2^31: the unsigned compare sends a negative index above every n)
__global__ void __launch_bounds__(256) k_permute_points(const uint4 *__restrict__ pts, uint32_t n, const int32_t *__restrict__ index,
                                                        uint4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = (uint32_t)index[i];
    const uint32_t q = 0x7FC00000u;
    out[i] = j < n ? pts[j] : make_uint4(q, q, q, q);
}

__global__ void __launch_bounds__(256) k_shuffle_points(const uint4 *__restrict__ pts, uint32_t n, ShuffleKeys keys, int h,
                                                        uint32_t mask, uint4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t x = feistel(i, keys, h, mask);
    while (x >= n) x = feistel(x, keys, h, mask);          // (ends: i < n lies on the cycle of x)
    out[i] = pts[x];
}

inline bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool bytes_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a_bytes > 0 && b_bytes > 0 && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

}  // namespace

extern "C" int vn_permute_points(const float *points, int64_t n, const int32_t *index, float *out, vnStream stream) {
    VN_CHECK_ARG(n >= 0 && n < (1ll << 31));
    if (n == 0) return VN_OK;
    VN_CHECK_ARG(points && index && out);
    VN_CHECK_ARG(!bytes_overlap(out, (size_t)n * 16, points, (size_t)n * 16));      // a gather cannot run in place
    VN_CHECK_ARG(!bytes_overlap(out, (size_t)n * 16, index, (size_t)n * 4));
    if (misaligned(points, 16) || misaligned(out, 16) || misaligned(index, 4)) return VN_EUNSUPPORTED;
    k_permute_points<<<(int)vn_ceil_div(n, 256), 256, 0, vn_stream(stream)>>>(reinterpret_cast<const uint4 *>(points), (uint32_t)n, index,
                                                                              reinterpret_cast<uint4 *>(out));
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" int vn_shuffle_points(const float *points, int64_t n, const uint32_t keys[6], float *out, vnStream stream) {
    VN_CHECK_ARG(n >= 0 && n < (1ll << 31));
    if (n == 0) return VN_OK;
    VN_CHECK_ARG(points && keys && out);
    VN_CHECK_ARG(!bytes_overlap(out, (size_t)n * 16, points, (size_t)n * 16));
    if (misaligned(points, 16) || misaligned(out, 16)) return VN_EUNSUPPORTED;
    int k = 0;                                              // bit_length(n - 1)
    for (uint64_t v = (uint64_t)(n - 1); v; v >>= 1) ++k;
    if (k < 2) k = 2;
    const int h = (k + 1) / 2;                              // k <= 31, so 2h <= 32
    const uint32_t mask = (1u << h) - 1u;
    ShuffleKeys kv;
    for (int r = 0; r < 6; ++r) kv.k[r] = keys[r];
    k_shuffle_points<<<(int)vn_ceil_div(n, 256), 256, 0, vn_stream(stream)>>>(reinterpret_cast<const uint4 *>(points), (uint32_t)n, kv, h,
                                                                              mask, reinterpret_cast<uint4 *>(out));
    VN_LAUNCH_STATUS();
    return VN_OK;
}
