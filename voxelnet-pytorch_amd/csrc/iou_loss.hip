// Rotated-IoU regression loss of the RPN: 1 - IoU ("iou") or 1 - IoU + rho2 / c2 ("diou") between the box an
// anchor's regression channels decode to and the box its target decodes to, bird's-eye view or 3D, forward and backward in
// ONE pass over the (B, h, w) anchor sites in the shape of loss.hip's k_loss: one thread per site, 2 anchors x 7 channels.
//   decode(d, A): diag = sqrt(A.w^2 + A.l^2)
//                 (d0*diag + A.x, d1*diag + A.y, d2*A.h + A.z, exp(d3)*A.h, exp(d4)*A.w, exp(d5)*A.l, d6 + A.r)
//   P = decode(delta[b, a*7 : a*7+7, y, x], A),  G = decode(targets[b, y, x, a*7 : a*7+7], A),  m = pos[b, y, x, a]
//   loss = sum_b (1 / P_b) * sum m * L,  P_b = max(1, sum pos[b]);   mean_iou = (sum m * IoU) / max(1, sum m)
// Layouts: delta (B,14,h,w) fp32 NCHW, pos (B,h,w,2) and targets (B,h,w,14) fp32 channels-last, anchors (h*w*2, 7) float64.
// All geometry is float64 (the fp32 inputs widened exactly); only d_delta and out2 are fp32.  Work is done where m != 0
// only: a thread without a positive writes its 14 zeros and leaves.
// The value: IoU is box_iou_pair (common.h) itself — what scoring and NMS compute, bit for bit.
// The derivative of the footprints' intersection area I with respect to P = (x, y, w, l, r), G constant, is the boundary
// integral dI/dtheta = sum over P's four edges of the integral over the part of the edge inside G of (v_theta . n) ds: the
// part of an edge inside a rectangle is a closed-form Liang-Barsky clip in that rectangle's frame (no polygon), and per
// part of length len, outward normal n and midpoint mid (from P's centre): dx += n_x len, dy += n_y len, dr += len n.perp(mid),
// dl += len / 2 on the two edges whose normal lies along the length axis, dw += len / 2 on the other two.  In P's own frame
// the normals are the unit vectors and n.perp(mid) is E (1/2 - t_mid) on every edge (E: the edge's length).
// Where IoU is not smooth (coincident edges, touching boxes, P == G) the clip picks one side; every term stays finite.
// Sums: per-thread double -> per-workgroup slab rows -> one workgroup adds the rows in a fixed order (deterministic); the
// normaliser pre-pass, the workgroup sum, the final pass and the workspace carve are rpn_common.h's site-term scaffold.
#include "rpn_common.h"

namespace {

constexpr int IOU_THREADS = VN_SITE_THREADS;

struct IouGeom {
    int32_t B, H, W, kind, metric;
};

// Liang-Barsky on one axis: the part of a + t d, t in [t0, t1], with |a + t d| <= h; t1 <= t0 afterwards when nothing is left
__device__ __forceinline__ void clip_axis(double a, double d, double h, double &t0, double &t1) {
    if (d == 0.0) {
        if (!(a >= -h && a <= h)) t1 = t0;
        return;
    }
    const double u = (-h - a) / d, v = (h - a) / d;
    t0 = fmax(t0, d > 0.0 ? u : v);
    t1 = fmin(t1, d > 0.0 ? v : u);
}

// One anchor: -> iou, L and (BWD) dL / d delta[0..7).  dp / dg: the seven regression channels and their targets, A: the anchor.
// An invalid pair — a decoded field not finite, a size not > 0, an area / volume sum not finite (the denominator is then
// not a number to divide by) — scores IoU 0, L = 1, gradient 0 in both kinds, the distance term skipped as well.
template <bool BWD>
__device__ __forceinline__ void iou_pair_loss(const double (&dp)[7], const double (&dg)[7], const double (&A)[7], int kind, int metric,
                                              double &iou, double &loss, double (&grad)[7]) {
    iou = 0.0;
    loss = 1.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) grad[k] = 0.0;
    double P[7], G[7], diag, S, V, ib, i3;
    if (!vn_iou_pair_value(dp, dg, A, metric, diag, P, G, S, V, ib, i3)) return;          // (rpn_common.h: the value half)
    const double area_p = P[4] * P[5];
    iou = metric == VN_IOU_3D ? i3 : ib;
    loss = 1.0 - iou;
    const double ptop = P[2] + P[3], gtop = G[2] + G[3];
    // gp: dL / d(x, y, z, h, w, l, r) of P
    double gp[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double cp = cos(P[6]), sp = sin(P[6]);
    if (BWD && iou > 0.0) {
        // P's corners (+,+), (-,+), (-,-), (+,-) in G's frame: G's centre the origin, G's length axis the first one
        const double cg = cos(G[6]), sg = sin(G[6]), cd = cos(P[6] - G[6]), sd = sin(P[6] - G[6]);
        const double ox = (P[0] - G[0]) * cg + (P[1] - G[1]) * sg, oy = -((P[0] - G[0]) * sg) + (P[1] - G[1]) * cg;
        const double sx[4] = {1.0, -1.0, -1.0, 1.0}, sy[4] = {1.0, 1.0, -1.0, -1.0};
        double qx[4], qy[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double u = sx[k] * (P[5] / 2), v = sy[k] * (P[4] / 2);
            qx[k] = ox + (u * cd - v * sd);
            qy[k] = oy + (u * sd + v * cd);
        }
        // edge k: corner k -> corner k + 1; outward normals in P's frame (0,1), (-1,0), (0,-1), (1,0)
        double len[4], dIr = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int n = (k + 1) & 3;
            double t0 = 0.0, t1 = 1.0;
            clip_axis(qx[k], qx[n] - qx[k], G[5] / 2, t0, t1);
            clip_axis(qy[k], qy[n] - qy[k], G[4] / 2, t0, t1);
            const double E = (k & 1) ? P[4] : P[5];
            len[k] = 0.0;
            if (t1 > t0) {
                len[k] = (t1 - t0) * E;
                dIr += len[k] * (E * (0.5 - 0.5 * (t0 + t1)));
            }
        }
        const double lx = len[3] - len[1], ly = len[0] - len[2];          // (dI/dx, dI/dy) in P's frame
        const double dIx = lx * cp - ly * sp, dIy = lx * sp + ly * cp;
        const double dIl = 0.5 * (len[1] + len[3]), dIw = 0.5 * (len[0] + len[2]);
        if (metric == VN_IOU_3D) {
            // iou3 = I3 / (V - I3), I3 = I zo:  d iou3 = (1 + iou3)^2 / V dI3 - iou3 (1 + iou3) / V dV
            const double I = ib * S / (1.0 + ib);
            const double zo = fmax(0.0, fmin(ptop, gtop) - fmax(P[2], G[2]));
            const double kI = (1.0 + i3) * (1.0 + i3) / V, kV = i3 * (1.0 + i3) / V;
            const double top_p = (zo > 0.0 && ptop < gtop) ? 1.0 : 0.0, bot_p = (zo > 0.0 && P[2] > G[2]) ? 1.0 : 0.0;
            gp[0] = -(kI * zo * dIx);
            gp[1] = -(kI * zo * dIy);
            gp[2] = -(kI * I * (top_p - bot_p));
            gp[3] = -(kI * I * top_p - kV * area_p);
            gp[4] = -(kI * zo * dIw - kV * (P[3] * P[5]));
            gp[5] = -(kI * zo * dIl - kV * (P[3] * P[4]));
            gp[6] = -(kI * zo * dIr);
        } else {
            // iou = I / (S - I):  d iou = (1 + iou)^2 / S dI - iou (1 + iou) / S dS
            const double kI = (1.0 + ib) * (1.0 + ib) / S, kS = ib * (1.0 + ib) / S;
            gp[0] = -(kI * dIx);
            gp[1] = -(kI * dIy);
            gp[4] = -(kI * dIw - kS * P[5]);
            gp[5] = -(kI * dIl - kS * P[4]);
            gp[6] = -(kI * dIr);
        }
    }
    if (kind == VN_IOU_LOSS_DIOU) {
        // the axis-aligned rectangle around the 8 footprint corners, P's centre the origin; which corner holds each side
        const double cg = cos(G[6]), sg = sin(G[6]);
        const double ddx = G[0] - P[0], ddy = G[1] - P[1];
        const double sx[4] = {1.0, -1.0, -1.0, 1.0}, sy[4] = {1.0, 1.0, -1.0, -1.0};
        double xmax = 0.0, xmin = 0.0, ymax = 0.0, ymin = 0.0;
        int kxmax = 0, kxmin = 0, kymax = 0, kymin = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool isp = k < 4;
            const double u = sx[k & 3] * ((isp ? P[5] : G[5]) / 2), v = sy[k & 3] * ((isp ? P[4] : G[4]) / 2);
            const double x = isp ? u * cp - v * sp : ddx + (u * cg - v * sg);
            const double y = isp ? u * sp + v * cp : ddy + (u * sg + v * cg);
            if (k == 0 || x > xmax) { xmax = x; kxmax = k; }
            if (k == 0 || x < xmin) { xmin = x; kxmin = k; }
            if (k == 0 || y > ymax) { ymax = y; kymax = k; }
            if (k == 0 || y < ymin) { ymin = y; kymin = k; }
        }
        const double ex = xmax - xmin, ey = ymax - ymin;
        double rho2 = ddx * ddx + ddy * ddy, c2 = ex * ex + ey * ey;
        double ddz = 0.0, ez = 0.0;
        if (metric == VN_IOU_3D) {
            ddz = (G[2] + G[3] / 2) - (P[2] + P[3] / 2);
            ez = fmax(ptop, gtop) - fmin(P[2], G[2]);
            rho2 += ddz * ddz;
            c2 += ez * ez;
        }
        if (isfinite(rho2) && isfinite(c2) && c2 > 0.0) {
            const double dist = rho2 / c2;
            loss += dist;
            if (BWD) {
                // d dist = (d rho2 - dist d c2) / c2; a side held by a corner of G does not move
                double dc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};          // d c2 / d(x, y, z, h, w, l, r) / 2
                const int ks[4] = {kxmax, kxmin, kymax, kymin};
                const double ext[4] = {ex, -ex, ey, -ey};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int k = ks[s];
                    if (k < 4) {
                        const double fx = k == 0 || k == 3 ? 1.0 : -1.0, fy = k < 2 ? 1.0 : -1.0;
                        const double u = fx * (P[5] / 2), v = fy * (P[4] / 2);
                        if (s < 2) {          // x = Px + u cos r - v sin r
                            dc[0] += ext[s];
                            dc[5] += ext[s] * (fx * cp / 2);
                            dc[4] += ext[s] * (-(fy * sp) / 2);
                            dc[6] += ext[s] * (-(u * sp + v * cp));
                        } else {              // y = Py + u sin r + v cos r
                            dc[1] += ext[s];
                            dc[5] += ext[s] * (fx * sp / 2);
                            dc[4] += ext[s] * (fy * cp / 2);
                            dc[6] += ext[s] * (u * cp - v * sp);
                        }
                    }
                }
                double dr[7] = {-2.0 * ddx, -2.0 * ddy, 0.0, 0.0, 0.0, 0.0, 0.0};          // d rho2
                if (metric == VN_IOU_3D) {
                    const double top_p = ptop > gtop ? 1.0 : 0.0, bot_p = P[2] < G[2] ? 1.0 : 0.0;
                    dc[2] += ez * (top_p - bot_p);
                    dc[3] += ez * top_p;
                    dr[2] = -2.0 * ddz;
                    dr[3] = -ddz;
                }
#pragma unroll
                for (int k = 0; k < 7; ++k) gp[k] += (dr[k] - dist * (2.0 * dc[k])) / c2;
            }
        }
    }
    if (BWD) {
        // through the decode: dPx/dd0 = diag, dPz/dd2 = A.h, dPh/dd3 = Ph, ...
        grad[0] = gp[0] * diag;
        grad[1] = gp[1] * diag;
        grad[2] = gp[2] * A[3];
        grad[3] = gp[3] * P[3];
        grad[4] = gp[4] * P[4];
        grad[5] = gp[5] * P[5];
        grad[6] = gp[6];
    }
}

template <bool BWD>
__global__ void __launch_bounds__(IOU_THREADS) k_iou_loss(const float *__restrict__ delta, const float *__restrict__ pos,
                                                          const float *__restrict__ tgt, const double *__restrict__ anchors,
                                                          const double *__restrict__ part, IouGeom g, const float *__restrict__ gup,
                                                          double *__restrict__ slab /* [blocks][3] */, float *__restrict__ d_delta) {
    VN_PRIO_MAIN();
    const int64_t hw = (int64_t)g.H * g.W, sites = hw * g.B;
    const int64_t site = (int64_t)blockIdx.x * IOU_THREADS + threadIdx.x;
    double s_loss = 0.0, s_iou = 0.0, s_m = 0.0;
    if (site < sites) {
        const int b = (int)(site / hw);
        const int64_t yx = site - (int64_t)b * hw;
        const float2 ps = *reinterpret_cast<const float2 *>(pos + site * 2);
#pragma unroll 1
        for (int a = 0; a < 2; ++a) {
            const float m = a ? ps.y : ps.x;
            float out[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (m != 0.f) {
                double dp[7], dg[7], A[7], grad[7], iou, L;
#pragma unroll
                for (int j = 0; j < 7; ++j) {
                    dp[j] = (double)delta[((int64_t)b * 14 + a * 7 + j) * hw + yx];
                    dg[j] = (double)tgt[site * 14 + a * 7 + j];
                    A[j] = anchors[(yx * 2 + a) * 7 + j];
                }
                iou_pair_loss<BWD>(dp, dg, A, g.kind, g.metric, iou, L, grad);
                const double wgt = (double)m / fmax(vn_pos_total(part, b), 1.0);
                s_loss += wgt * L;
                s_iou += (double)m * iou;
                s_m += (double)m;
                if (BWD) {
                    const double k = wgt * (gup ? (double)*gup : 1.0);
#pragma unroll
                    for (int j = 0; j < 7; ++j) out[j] = (float)(k * grad[j]);
                }
            }
            if (BWD) {
#pragma unroll
                for (int j = 0; j < 7; ++j) d_delta[((int64_t)b * 14 + a * 7 + j) * hw + yx] = out[j];
            }
        }
    }
    const double t = vn_block_sum3<IOU_THREADS>(s_loss, s_iou, s_m);
    if (threadIdx.x < 3) slab[(int64_t)blockIdx.x * 3 + threadIdx.x] = t;
}

}  // namespace

extern "C" size_t vn_rpn_iou_loss_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    return vn_site_map_ok(B, H, W) ? VnSiteTermWs(B, H, W).bytes() : 0;
}

extern "C" int vn_rpn_iou_loss(const float *delta, const float *pos, const float *targets, const double *anchors, int32_t B,
                               int32_t H, int32_t W, int32_t kind, int32_t metric, const float *g, void *workspace,
                               size_t workspace_bytes, float *out2, float *d_delta, vnStream stream) {
    VN_CHECK_ARG(vn_site_map_ok(B, H, W));
    VN_CHECK_ARG(kind == VN_IOU_LOSS_IOU || kind == VN_IOU_LOSS_DIOU);
    VN_CHECK_ARG(metric == VN_IOU_BEV || metric == VN_IOU_3D);
    VN_CHECK_ARG(delta && pos && targets && anchors && workspace && out2);
    const VnSiteTermWs ws(B, H, W);
    if (workspace_bytes < ws.bytes()) return VN_EWORKSPACE;
    hipStream_t st = vn_stream(stream);
    double *part = ws.part(workspace), *slab = ws.slab(workspace);
    k_pos_norm<VN_SITE_THREADS><<<B * VN_POS_CHUNKS, VN_SITE_THREADS, 0, st>>>(pos, (int64_t)H * W * 2, part);
    VN_LAUNCH_STATUS();
    const IouGeom geom{B, H, W, kind, metric};
    if (d_delta)
        k_iou_loss<true><<<ws.blocks, IOU_THREADS, 0, st>>>(delta, pos, targets, anchors, part, geom, g, slab, d_delta);
    else
        k_iou_loss<false><<<ws.blocks, IOU_THREADS, 0, st>>>(delta, pos, targets, anchors, part, geom, g, slab, nullptr);
    VN_LAUNCH_STATUS();
    k_site_term_finalize<VN_SITE_THREADS><<<1, VN_SITE_THREADS, 0, st>>>(slab, ws.blocks, out2);
    VN_LAUNCH_STATUS();
    return VN_OK;
}
