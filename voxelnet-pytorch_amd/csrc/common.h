// Shared helpers for the gfx950 kernels.  Wave = 64 lanes everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/voxelnet_hip.h"

#define VN_WAVE 64

#define VN_CHECK_ARG(cond) do { if (!(cond)) return VN_EINVAL; } while (0)
#define VN_LAUNCH_STATUS() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)
#define VN_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return (int)e_; } while (0)

// Tuning aids: the ONLY way this library reads the environment.  vn_knob(name, default) returns the integer value of the
// environment variable `name` if it is set (and listed in abi.hip's table: an unlisted name always returns the default),
// else `default`; callers keep the result in a function-local static (read once per process).  vn_build_info() reports
// every listed variable that is set, so a stray VN_* in the environment shows up in bench.py's JSON line.
int vn_knob(const char *name, int dflt);
// fp32x3: a conv weight operand with rows of K channels holds hi / lo bf16 granules (vn_pack_weight, VN_F32X3) when K is a
// whole number of 32-channel chunks; other K (the heads' 16-column data-gradient operand) stay fp32 and are split in registers.
// The packer and the convolution entry points both ask here.
inline bool vn_x3_presplit(int K) { return K > 0 && K % 32 == 0; }

static inline hipStream_t vn_stream(vnStream s) { return reinterpret_cast<hipStream_t>(s); }
static inline int64_t vn_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t vn_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Wave priority of the kernels on the step's dependency chain (convolutions, BatchNorm passes, VFE, loss): the weight
// gradients of the side stream keep the default 0.  Two waves of different kernels on one SIMD are arbitrated by priority,
// then AGE (MI355X_MICROARCH.md, "Two waves per SIMD"): the long-lived weight-gradient waves are always the older ones, so
// at equal priority the chain's short kernels lose every issue slot they contend for.  -DVN_MAIN_PRIO=n builds set
// s_setprio n at the top of those kernels (round 4 A/B; 0 / undefined = no instruction).
#if defined(VN_MAIN_PRIO) && VN_MAIN_PRIO > 0
#define VN_PRIO_MAIN() __builtin_amdgcn_s_setprio(VN_MAIN_PRIO)
#else
#define VN_PRIO_MAIN() ((void)0)
#endif

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

// fp32 -> bf16 round-to-nearest-even via the hardware cast (keeps NaN a NaN)
__device__ __forceinline__ bf16_t vn_f2bf(float x) { return (bf16_t)x; }
__device__ __forceinline__ float vn_bf2f(bf16_t x) { return (float)x; }

// bf16x3 split: x ~= hi + lo with hi = bf16(x), lo = bf16(x - hi)
__device__ __forceinline__ void vn_split_bf16(float x, bf16_t &hi, bf16_t &lo) {
    hi = (bf16_t)x;
    lo = (bf16_t)(x - (float)hi);
}

// "fp32x3" products (vnDtype VN_F32X3: fp32 storage, every product as three bf16 MFMAs): eight fp32 operands of a lane ->
// hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32); a.b ~= ah.bh + al.bh + ah.bl, error ~2^-16 per product
__device__ __forceinline__ void vn_split8(const float (&v)[8], bf16x8_t &hi, bf16x8_t &lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const bf16_t h = (bf16_t)v[e];
        hi[e] = h;
        lo[e] = (bf16_t)(v[e] - (float)h);
    }
}
__device__ __forceinline__ void vn_split8(const f32x4_t &a0, const f32x4_t &a1, bf16x8_t &hi, bf16x8_t &lo) {
    const float v[8] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
    vn_split8(v, hi, lo);
}
__device__ __forceinline__ f32x4_t vn_mfma_x3(const bf16x8_t &ah, const bf16x8_t &al, const bf16x8_t &bh, const bf16x8_t &bl, f32x4_t c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, c, 0, 0, 0);
}

__device__ __forceinline__ float vn_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float vn_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int vn_wave_min_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- ordered compaction (count per workgroup -> one-workgroup exclusive scan of the counts -> write each survivor at
// its scanned position), shared by fov.hip, gtsample.hip, voxelize.hip and sparse.hip.
// Workgroup-wide exclusive scan of one value per thread (THREADS threads, all of which must reach it): returns the
// exclusive prefix, *total = the workgroup's sum.  The trailing barrier lets a caller call it again in a loop.
template <typename T, int THREADS>
__device__ T vn_block_excl_scan(T v, T *total) {
    static_assert(THREADS % VN_WAVE == 0, "whole waves");
    __shared__ T wsum[THREADS / VN_WAVE];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < THREADS / VN_WAVE; ++w) {
        const T s = wsum[w];
        if (w < wid) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// One workgroup of THREADS threads: exclusive scan of blk[0..nb) in place, THREADS sums per trip with a running carry;
// returns the grand total to every thread.  nb == 0 returns 0 and touches nothing.
template <typename T, int THREADS>
__device__ T vn_scan_block_sums(T *blk, int64_t nb) {
    T carry = 0;
    for (int64_t base = 0; base < nb; base += THREADS) {
        const int64_t i = base + threadIdx.x;
        const T v = i < nb ? blk[i] : T(0);
        T tot;
        const T ex = vn_block_excl_scan<T, THREADS>(v, &tot);
        if (i < nb) blk[i] = carry + ex;
        carry += tot;
    }
    return carry;
}

// 256-thread workgroup, one flag per thread (wave ballot + popcount, the four wave counts through LDS): the exclusive
// rank of this thread among the threads whose `keep` is set; *total (optional) = how many are set.  Every thread of the
// workgroup must reach it (it holds a barrier), and a kernel calls it once: nothing guards wsum against a second call.
__device__ __forceinline__ int vn_block_rank(bool keep, int *total = nullptr) {
    __shared__ int wsum[256 / VN_WAVE];
    const unsigned long long m = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 256 / VN_WAVE; ++w) {
        const int s = wsum[w];
        if (w < wave) base += s;
        tot += s;
    }
    if (total) *total = tot;
    return base + __popcll(m & ((1ull << lane) - 1ull));
}
__device__ __forceinline__ int vn_block_count(bool keep) {
    int total;
    vn_block_rank(keep, &total);
    return total;
}

// The point-in-rotated-box test of gtsample.hip and of augment.hip's composed pass, one copy: Box = vnGtBox or a struct
// that begins with its eight fields (vnObjectMove).  float64 exactly as written, inclusive; a NaN anywhere fails.
template <typename Box>
__device__ __forceinline__ bool vn_gt_inside(double px, double py, double pz, const Box &q) {
    const double dx = px - q.x, dy = py - q.y;
    const double u = dx * q.c + dy * q.s;
    const double v = -(dx * q.s) + dy * q.c;
    return fabs(u) <= q.hl && fabs(v) <= q.hw && pz >= q.z0 && pz <= q.z1;
}

// The 32-bit finalizer of MurmurHash3, as include/voxelnet_hip.h writes it: the round function of shuffle.hip's keyed
// bijection and the per-row hash of part_augment.hip's thinning.  Exact uint32 arithmetic (wrapping multiplies).
__device__ __forceinline__ uint32_t vn_fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// Buffer descriptor from values the compiler can PROVE wave-uniform (cdna_hip_programming.md T20): without
// the readfirstlane of the pointer halves and the size, hipcc wraps every buffer_load ... lds that uses the
// descriptor in a waterfall loop (v_readfirstlane x4 + s_and_saveexec + loop), ~15 instructions and a
// serialisation point per load.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t vn_uniform_rsrc(const void *base, uint32_t bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    const uint32_t n = __builtin_amdgcn_readfirstlane(bytes);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((uint64_t)hi << 32) | lo), 0, (int)n, 0x00020000);
}

// ---- rotated-box pair IoU, shared by eval.hip (scoring) and detect.hip (rotated NMS).  Box =
// (x, y, z, h, w, l, r); float64 throughout; the clipped polygon lives in registers (fixed-index unrolled loops, see eval.hip).
constexpr int EV_NV = 8;          // vertices of a rectangle clipped by a rectangle

__device__ __forceinline__ void poly_push(double (&px)[EV_NV], double (&py)[EV_NV], int &n, double x, double y) {
#pragma unroll
    for (int j = 0; j < EV_NV; ++j) {
        const bool here = (j == n);
        px[j] = here ? x : px[j];
        py[j] = here ? y : py[j];
    }
    ++n;
}

// keep the part of the polygon on the left of the directed line through (ex, ey) with direction (dx, dy)
__device__ __forceinline__ void clip_halfplane(const double (&ix)[EV_NV], const double (&iy)[EV_NV], int n, double ex, double ey,
                                               double dx, double dy, double (&ox)[EV_NV], double (&oy)[EV_NV], int &m) {
    m = 0;
#pragma unroll
    for (int j = 0; j < EV_NV; ++j) { ox[j] = 0.0; oy[j] = 0.0; }
    double px = ix[0], py = iy[0];          // the last vertex: the walk starts on the edge last -> first
#pragma unroll
    for (int j = 1; j < EV_NV; ++j) {
        const bool last = (j == n - 1);
        px = last ? ix[j] : px;
        py = last ? iy[j] : py;
    }
    double dp = dx * (py - ey) - dy * (px - ex);
#pragma unroll
    for (int i = 0; i < EV_NV; ++i) {
        if (i < n) {
            const double cx = ix[i], cy = iy[i];
            const double dc = dx * (cy - ey) - dy * (cx - ex);
            if ((dp >= 0.0) != (dc >= 0.0)) {
                const double t = dp / (dp - dc);
                poly_push(ox, oy, m, px + (cx - px) * t, py + (cy - py) * t);
            }
            if (dc >= 0.0) poly_push(ox, oy, m, cx, cy);
            px = cx; py = cy; dp = dc;
        }
    }
}

__device__ __forceinline__ bool box_ok(const double (&q)[7]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) ok = ok && isfinite(q[k]);
    return ok && q[3] > 0.0 && q[4] > 0.0 && q[5] > 0.0;
}

// the ONE pair function: vn_box_iou_rotated and vn_eval_match both call it
__device__ __forceinline__ void box_iou_pair(const double (&a)[7], const double (&b)[7], double &iou_bev, double &iou_3d) {
    iou_bev = 0.0;
    iou_3d = 0.0;
    if (!(box_ok(a) && box_ok(b))) return;
    const double ca = cos(a[6]), sa = sin(a[6]), cb = cos(b[6]), sb = sin(b[6]);
    const double la = a[5] / 2, wa = a[4] / 2, lb = b[5] / 2, wb = b[4] / 2;
    const double ox = b[0] - a[0], oy = b[1] - a[1];          // B's centre seen from A's
    // counter-clockwise corners (+,+), (-,+), (-,-), (+,-) of the local (l, w) frame, turned by r
    const double sx[4] = {1.0, -1.0, -1.0, 1.0}, sy[4] = {1.0, 1.0, -1.0, -1.0};
    double p0x[EV_NV], p0y[EV_NV], p1x[EV_NV], p1y[EV_NV], bx[4], by[4];
#pragma unroll
    for (int k = 0; k < EV_NV; ++k) { p0x[k] = 0.0; p0y[k] = 0.0; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double ax = sx[k] * la, ay = sy[k] * wa;
        p0x[k] = ax * ca - ay * sa;
        p0y[k] = ax * sa + ay * ca;
        const double qx = sx[k] * lb, qy = sy[k] * wb;
        bx[k] = (qx * cb - qy * sb) + ox;
        by[k] = (qx * sb + qy * cb) + oy;
    }
    int n = 4, m = 0;
    clip_halfplane(p0x, p0y, n, bx[0], by[0], bx[1] - bx[0], by[1] - by[0], p1x, p1y, m);
    clip_halfplane(p1x, p1y, m, bx[1], by[1], bx[2] - bx[1], by[2] - by[1], p0x, p0y, n);
    clip_halfplane(p0x, p0y, n, bx[2], by[2], bx[3] - bx[2], by[3] - by[2], p1x, p1y, m);
    clip_halfplane(p1x, p1y, m, bx[3], by[3], bx[0] - bx[3], by[0] - by[3], p0x, p0y, n);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < EV_NV; ++i) {
        if (i < n) {
            const bool wrap = (i + 1 >= n);          // the closing edge: last -> first
            const double nx = wrap ? p0x[0] : p0x[(i + 1) % EV_NV];
            const double ny = wrap ? p0y[0] : p0y[(i + 1) % EV_NV];
            s += p0x[i] * ny - nx * p0y[i];
        }
    }
    const double inter = 0.5 * fabs(s);
    const double area_a = a[4] * a[5], area_b = b[4] * b[5];
    const double den2 = area_a + area_b - inter;
    iou_bev = den2 > 0.0 ? inter / den2 : 0.0;
    const double zo = fmax(0.0, fmin(a[2] + a[3], b[2] + b[3]) - fmax(a[2], b[2]));
    const double inter3 = inter * zo;
    const double den3 = a[3] * area_a + b[3] * area_b - inter3;
    iou_3d = den3 > 0.0 ? inter3 / den3 : 0.0;
}
