// Point-cloud augmentation of the input pipeline — the per-point half of the reference's `pcl_augmentation`
// (voxelnet/dataset.py:122-219: per-box perturbation, global rotation, global scaling — paper section 3.2; the moves
// themselves are `point_transform`, dataset.py:264, and `box_transform`, :254).  The O(boxes) half — the random draw,
// the collision test (`calc_iou2d`, :222-240) and the moved labels (`corner_to_center_box3d`, :305-384) — stays on the
// host (voxelnet_amd/augment.py); this file moves the points, between the optional field-of-view crop and the
// voxelizer, on the pipeline's stream.
//
// The rigid motion is the reference's `point_transform`: translate, then multiply the ROW vector by the z-rotation
// matrix — a rotation by -rz about the lidar origin:
//   X = x + tx, Y = y + ty, Z = z + tz;   x' = X*c + Y*s,  y' = -(X*s) + Y*c,  z' = Z      (c = cos rz, s = sin rz)
// evaluated in float64 exactly as written (no contraction: the Makefile builds with -ffp-contract=off) and rounded once
// to float32; c and s come from the host, so the device result does not depend on a device sin / cos.
//   boxes mode : a point walks the table in index order ON ITS CURRENT VALUE and is moved by every box whose float32
//                bounds contain it (inclusive) — the reference's in-place loop over boxes; each point's fate is
//                independent of every other point's, so one thread per point reproduces it exactly
//   rotate mode: the motion with t = 0 for every point
//   scale mode : one float32 multiply per coordinate
// Reflectance is copied.  A NaN point (the padding rows of vn_fov_crop) fails every bounds test and stays NaN in the
// other two modes, so the voxelizer still drops it.
// Memory-bound by construction: 16 B read + 16 B written per point, the table (<= 8 KB) staged once per workgroup in
// LDS, float64 only inside the taken branch.
//
// The composed recipe (SECOND / PointPillars: per-object noise, flip, global rotation, scaling, translation — DESIGN.md
// section 1a-quater) is a second entry point of this file, vn_augment_compose, one launch for all five stages:
//   membership : vn_gt_inside (common.h, gtsample.hip's rotated-box test) of the ORIGINAL point in the unmoved boxes; the
//                lowest entry that holds the point wins and a point takes AT MOST ONE object move
//   object move: the point turns about ITS box's centre, then travels with it
//                  X = (x + tx) + (dx*rc - dy*rs),  Y = (y + ty) + (dx*rs + dy*rc),  Z = pz + tz
//   affine     : x' = (a00*X + a01*Y) + bx,  y' = (a10*X + a11*Y) + by,  z' = sz*Z + bz          for every point
// in float64 as written, rounded once; a NaN coordinate is in no box and stays NaN through the affine.  16 B read + 16 B
// written per point, the table (<= 16 KB) staged once per workgroup in LDS and read at wave-uniform addresses.
#include "common.h"

namespace {

static_assert(sizeof(vnAugmentBox) == 64, "vnAugmentBox is four 16-byte words");
static_assert(sizeof(vnObjectMove) == 128 && sizeof(vnAffine) == 64, "vnObjectMove is eight 16-byte words");

__device__ __forceinline__ void rigid_motion(float4 &p, double tx, double ty, double tz, double c, double s) {
    const double X = (double)p.x + tx, Y = (double)p.y + ty, Z = (double)p.z + tz;
    p.x = (float)(X * c + Y * s);
    p.y = (float)(-(X * s) + Y * c);
    p.z = (float)Z;
}

// (pts / out carry no __restrict__: out may BE pts — every thread reads its own row, then writes the same row)
__global__ void __launch_bounds__(256) k_augment_boxes(const float4 *pts, int64_t n, const vnAugmentBox *__restrict__ boxes,
                                                       int n_boxes, float4 *out) {
    __shared__ __attribute__((aligned(16))) vnAugmentBox tab[VN_AUGMENT_MAX_BOXES];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(boxes);
        uint4 *dst = reinterpret_cast<uint4 *>(tab);
        for (int w = threadIdx.x; w < n_boxes * 4; w += 256) dst[w] = src[w];
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 p = pts[i];
    for (int b = 0; b < n_boxes; ++b) {
        const vnAugmentBox &q = tab[b];          // (wave-uniform address: an LDS broadcast)
        if (p.x >= q.lo[0] && p.x <= q.hi[0] && p.y >= q.lo[1] && p.y <= q.hi[1] && p.z >= q.lo[2] && p.z <= q.hi[2])
            rigid_motion(p, q.tx, q.ty, q.tz, q.c, q.s);
    }
    out[i] = p;
}

__global__ void __launch_bounds__(256) k_augment_rotate(const float4 *pts, int64_t n, double c, double s, float4 *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 p = pts[i];
    rigid_motion(p, 0.0, 0.0, 0.0, c, s);
    out[i] = p;
}

__global__ void __launch_bounds__(256) k_augment_scale(const float4 *pts, int64_t n, float f, float4 *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 p = pts[i];
    p.x *= f;
    p.y *= f;
    p.z *= f;
    out[i] = p;
}

__global__ void __launch_bounds__(256) k_augment_compose(const float4 *pts, int64_t n, const vnObjectMove *__restrict__ moves,
                                                         int n_moves, vnAffine a, float4 *out) {
    __shared__ __attribute__((aligned(16))) vnObjectMove tab[VN_AUGMENT_MAX_BOXES];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(moves);
        uint4 *dst = reinterpret_cast<uint4 *>(tab);
        for (int w = threadIdx.x; w < n_moves * 8; w += 256) dst[w] = src[w];
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 p = pts[i];
    const double px = (double)p.x, py = (double)p.y, pz = (double)p.z;
    double X = px, Y = py, Z = pz;
    for (int b = 0; b < n_moves; ++b) {
        const vnObjectMove &q = tab[b];          // (wave-uniform address: an LDS broadcast)
        if (vn_gt_inside(px, py, pz, q)) {
            const double dx = px - q.x, dy = py - q.y;
            X = (q.x + q.tx) + (dx * q.rc - dy * q.rs);
            Y = (q.y + q.ty) + (dx * q.rs + dy * q.rc);
            Z = pz + q.tz;
            break;                               // the first hit ends the walk: at most one object move
        }
    }
    p.x = (float)((a.a00 * X + a.a01 * Y) + a.bx);
    p.y = (float)((a.a10 * X + a.a11 * Y) + a.by);
    p.z = (float)(a.sz * Z + a.bz);
    out[i] = p;
}

}  // namespace

extern "C" int vn_augment_compose(const float *points, int64_t n, const vnObjectMove *moves, int32_t n_moves,
                                  const vnAffine *affine, float *out, vnStream stream) {
    VN_CHECK_ARG(n >= 0 && n < (1ll << 31));
    VN_CHECK_ARG(n_moves >= 0 && n_moves <= VN_AUGMENT_MAX_BOXES);
    VN_CHECK_ARG(affine);
    VN_CHECK_ARG(n_moves == 0 || moves);
    if (n == 0) return VN_OK;
    VN_CHECK_ARG(points && out);
    if ((reinterpret_cast<uintptr_t>(points) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return VN_EUNSUPPORTED;
    if (n_moves > 0 && (reinterpret_cast<uintptr_t>(moves) & 15)) return VN_EUNSUPPORTED;
    k_augment_compose<<<(int)vn_ceil_div(n, 256), 256, 0, vn_stream(stream)>>>(reinterpret_cast<const float4 *>(points), n, moves,
                                                                                 n_moves, *affine, reinterpret_cast<float4 *>(out));
    VN_LAUNCH_STATUS();
    return VN_OK;
}

extern "C" int vn_augment_points(const float *points, int64_t n, int32_t mode, const vnAugmentBox *boxes, int32_t n_boxes,
                                 double c, double s, float scale, float *out, vnStream stream) {
    VN_CHECK_ARG(n >= 0 && n < (1ll << 31));
    VN_CHECK_ARG(mode == VN_AUGMENT_BOXES || mode == VN_AUGMENT_ROTATE || mode == VN_AUGMENT_SCALE);
    VN_CHECK_ARG(mode != VN_AUGMENT_BOXES || (n_boxes >= 0 && n_boxes <= VN_AUGMENT_MAX_BOXES));
    if (n == 0) return VN_OK;
    VN_CHECK_ARG(points && out);
    VN_CHECK_ARG(mode != VN_AUGMENT_BOXES || n_boxes == 0 || boxes);
    if ((reinterpret_cast<uintptr_t>(points) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return VN_EUNSUPPORTED;
    if (mode == VN_AUGMENT_BOXES && n_boxes > 0 && (reinterpret_cast<uintptr_t>(boxes) & 15)) return VN_EUNSUPPORTED;
    if (mode == VN_AUGMENT_BOXES && n_boxes == 0 && out == points) return VN_OK;      // nothing moves, nothing to copy
    hipStream_t st = vn_stream(stream);
    const int nb = (int)vn_ceil_div(n, 256);
    const float4 *src = reinterpret_cast<const float4 *>(points);
    float4 *dst = reinterpret_cast<float4 *>(out);
    if (mode == VN_AUGMENT_BOXES)
        k_augment_boxes<<<nb, 256, 0, st>>>(src, n, boxes, n_boxes, dst);
    else if (mode == VN_AUGMENT_ROTATE)
        k_augment_rotate<<<nb, 256, 0, st>>>(src, n, c, s, dst);
    else
        k_augment_scale<<<nb, 256, 0, st>>>(src, n, scale, dst);
    VN_LAUNCH_STATUS();
    return VN_OK;
}
