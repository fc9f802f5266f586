/*
 * voxelnet_hip.h — C ABI of libvoxelnet_hip.so (gfx950 / MI355X).
 *
 * The reference (johanngerberding/voxelnet-pytorch) has no FFI or operator
 * registry: its hot path is Python calling ATen/NumPy.  This header is the
 * boundary a maintainer would bind (ctypes stub in INTEGRATION.md) to replace
 * those calls; every entry point cites the reference code it stands in for
 * (paths relative to /root/reference/voxelnet/).
 *
 * Conventions:
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - every pointer is a DEVICE pointer unless the name ends in _host.
 *   - the library never allocates or frees caller-visible memory: outputs and
 *     workspaces are caller-allocated; *_workspace_bytes() say how much.
 *   - asynchronous: work is enqueued on `stream` (a hipStream_t passed as
 *     void*) and ordered only by it.  No entry point synchronises.
 *   - return value: 0 ok, <0 invalid argument (VN_E*), >0 a hipError_t.
 *   - no global mutable state; re-entrant.
 *   - activations are channels-last: (B, D, H, W, C) / (B, H, W, C).
 */
#ifndef VOXELNET_HIP_H
#define VOXELNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VN_OK 0
#define VN_EINVAL (-1)     /* bad argument (null pointer, negative size, ...) */
#define VN_EUNSUPPORTED (-2) /* shape outside what the kernels are built for */
#define VN_EWORKSPACE (-3) /* workspace too small */

typedef enum { VN_F32 = 0, VN_BF16 = 1,
               /* OPERAND dtype of the conv / weight-gradient entry points only (vnConv.dtype): fp32 storage — sources and
                * rows exactly as VN_F32 — with every product evaluated as three bf16 MFMAs on hi / lo splits (a.b ~=
                * ah.bh + al.bh + ah.bl, ~2^-16 per product): the "fp32x3" mode, ~1e-4 on the RPN maps at a fraction of the
                * exact fp32 MFMA cost (round 4).  Sources / rows are split in registers; PACKED WEIGHTS of a convolution
                * launched with this dtype must come from vn_pack_weight(s_batch) with packed_dtype VN_F32X3, which splits
                * them once (same bytes as fp32; the layout is described there).  Tensor dtypes (outputs, BatchNorm, ...)
                * never take this value. */
               VN_F32X3 = 2,
               /* "split fp32" STORAGE (round 5): a tensor of C % 8 == 0 channels at 4 bytes per element, every aligned group of 8
                * channels = 32 B holding the eight hi bf16 parts (hi = bf16(x)) followed by the eight lo parts (lo = bf16(x -
                * hi)) — x to ~2^-17, the precision the VN_F32X3 products use of an fp32 operand anyway.  Written by the
                * BatchNorm passes (vn_bn_apply / vn_bn_bwd_apply and their BEV forms: a_dtype / dy_dtype), read as vnConv.dtype
                * by the conv entry points (source rows; the packed weights are the VN_F32X3 ones, same format) and the
                * weight-gradient entry points (BOTH operands): the fp32x3 products without any split work in the kernels.
                * Element strides count 4-byte elements and must be multiples of 8; Cs % 32 == 0 for a convolution source. */
               VN_F32X3S = 3 } vnDtype;

typedef void *vnStream; /* hipStream_t */

int vn_abi_version(void); /* bumps when a signature, a data layout or a call protocol changes (4: round 5) */
const char *vn_build_info(void); /* "gfx950 <date> ..." static string */
const char *vn_build_id(void);   /* 12 hex digits: SHA-256 over the library's sources (changes with ANY source change) */

/* ------------------------------------------------------------------------
 * Voxelizer — utils.py:10-100 (pcl_to_voxels), minus the host-side shuffle
 * (utils.py:35), which the Python wrapper performs before upload.
 * Grid literals: utils.py:24-33.
 * ---------------------------------------------------------------------- */
typedef struct {
    int32_t D, H, W;   /* grid (z,y,x) */
    float vz, vy, vx;  /* voxel size (z,y,x), float32 as in the reference */
    float ox, oy, oz;  /* lidar_coord added to (x,y,z) */
    int32_t T;         /* max points per voxel (<= 64) */
} vnGrid;

size_t vn_voxelize_workspace_bytes(int64_t n_points, const vnGrid *grid);

/* Phase 1 (utils.py:37-63): per-point voxel key (exact fp32 add / IEEE divide /
 * floor), occupancy, ordered compaction.  Writes K (number of non-empty voxels,
 * rows sorted by z,y,x) to *k_out (device int32).  The caller reads K back
 * (one 4-byte copy) to size phase 2's outputs — the reference returns
 * (K,T,7)/(K,3)/(K,) arrays, so K is part of the boundary format. */
int vn_voxelize_index(const float *points /*[N,4]*/, int64_t n_points,
                      const vnGrid *grid, void *workspace, size_t workspace_bytes,
                      int32_t *k_out, vnStream stream);

/* Phase 2 (utils.py:69-88 + dataset.py:110-117): first-T points per voxel in
 * input order, centroid offsets on all T slots (float64 divide/subtract as
 * numpy promotes), int64 coordinates with `coord_cols` = 3 (z,y,x) or
 * 4 (batch_index,z,y,x; prepare_voxel's padding), int64 counts.
 * Deterministic: no order-dependent atomics reach the outputs.
 * k_dev == NULL: K is the exact row count (read back from phase 1).  k_dev != NULL
 * (phase 1's k_out): K is only the CAPACITY of the output buffers (any K <= n_points
 * fits) and rows >= *k_dev are left untouched — no host read-back between the phases. */
int vn_voxelize_gather(const float *points, int64_t n_points, const vnGrid *grid,
                       void *workspace, size_t workspace_bytes, int64_t K,
                       int64_t batch_index, int32_t coord_cols,
                       float *feature /*[K,T,7]*/, int64_t *coord /*[K,coord_cols]*/,
                       int64_t *number /*[K]*/, const int32_t *k_dev, vnStream stream);

/* Host (CPU) variant of the two phases for the reference's own call site — pcl_to_voxels inside forked DataLoader
 * worker processes (dataset.py:58, train.py:77-84), which cannot touch the GPU.  HOST pointers, no stream, synchronous;
 * same arithmetic, row order and output formats as the device pair above, bit for bit.  The index phase leaves its
 * row table in `workspace`; the gather phase must be given the K it returned. */
size_t vn_voxelize_host_workspace_bytes(int64_t n_points, const vnGrid *grid);
int vn_voxelize_host_index(const float *points /*host [N,4]*/, int64_t n_points, const vnGrid *grid,
                           void *workspace /*host*/, size_t workspace_bytes, int64_t *k_out);
int vn_voxelize_host_gather(const float *points, int64_t n_points, const vnGrid *grid, const void *workspace,
                            size_t workspace_bytes, int64_t K, int64_t batch_index, int32_t coord_cols,
                            float *feature /*host [K,T,7]*/, int64_t *coord /*host [K,coord_cols]*/,
                            int64_t *number /*host [K]*/);

/* ------------------------------------------------------------------------
 * Voxel feature encoder — FeatureLearningNet.forward up to the scatter
 * (model.py:93-100) incl. both VFELayer.forward calls (model.py:74-82):
 *   mask = max_c(x) != 0 ; h1 = relu(x W1^T + b1) ; p1 = BN1d(h1) over all K*T rows
 *   out1 = [p1, max_T p1] * mask ; h2 = relu(out1 W2^T + b2) ; p2 = BN1d(h2)
 *   out2 = [p2, max_T p2] * mask ; voxelwise = max_T out2            (K,128)
 * Shapes are the reference's: W1 (16,7), W2 (64,32), T <= 64.
 * Train mode uses batch statistics (biased variance) and updates the running
 * statistics (momentum, unbiased variance) exactly like nn.BatchNorm1d.
 * stats (320 floats: [mean|invstd|gamma*invstd|beta] of BN1 then BN2) is saved
 * for the backward.  Deterministic (fixed-order slab reductions, no float atomics).
 * ---------------------------------------------------------------------- */
typedef struct {
    const float *w1, *b1, *g1, *be1; float *rm1, *rv1;   /* vfe_1: fcn.0.weight/bias, bn.weight/bias, running stats */
    const float *w2, *b2, *g2, *be2; float *rm2, *rv2;   /* vfe_2 */
} vnVfeWeights;
typedef struct {
    float *dw1, *db1, *dg1, *dbe1, *dw2, *db2, *dg2, *dbe2;   /* overwritten */
} vnVfeGrads;

size_t vn_vfe_workspace_bytes(int64_t K, int32_t T);
int vn_vfe_fwd(const float *feature /*[K,T,7]*/, int64_t K, int32_t T, const vnVfeWeights *w,
               int32_t training, float momentum, float eps, float *voxelwise /*[K,128]*/,
               float *stats /*[320]*/, void *workspace, size_t workspace_bytes, vnStream stream);
/* vn_vfe_fwd that ALSO writes the voxel features as bf16 rows (K, 128) — bf16(x) of every element of `voxelwise`, what
 * vn_cast_rows makes of it — for a caller whose next consumer reads bf16 (vn_net_step in the bf16 mode: the first Conv3d's
 * rulebook GEMM; one launch less at the start of the step's dependency chain). */
int vn_vfe_fwd_rows(const float *feature, int64_t K, int32_t T, const vnVfeWeights *w, int32_t training, float momentum,
                    float eps, float *voxelwise, void *rows_bf16, float *stats, void *workspace, size_t workspace_bytes,
                    vnStream stream);
/* gradients of all eight parameter tensors for upstream d_voxelwise (K,128); the input
 * features are leaf data (no d_feature).  `workspace` need not be the forward's; when it IS — the buffer vn_vfe_fwd
 * was given for the same feature / K / T, untouched since — pass workspace_is_forwards = 1 (bit 0) and the effective-row
 * work list found there is reused instead of rebuilt (two launches less).  Bit 1 of workspace_is_forwards: the forward
 * ran with training = 0 (stats = the running statistics): the eval-mode BatchNorm backward, whose batch-statistic terms
 * vanish (the reference's autograd through `model.eval()`; model.py:76 with self.training False). */
int vn_vfe_bwd(const float *feature, int64_t K, int32_t T, const vnVfeWeights *w, const float *stats,
               const float *d_voxelwise, const vnVfeGrads *g, void *workspace,
               size_t workspace_bytes, int32_t workspace_is_forwards, vnStream stream);

/* Stand-alone VFELayer.forward(inputs, mask) (model.py:60-82) for callers that compose the layers themselves:
 * out (K,T,2*units) = concat(p, max_t p) * mask with p = BatchNorm1d(relu(inputs W^T + b)) over the K*T rows
 * (training: batch statistics + running-stat update with `momentum`; else the running statistics).  mask: one
 * byte per (voxel, slot) row.  cin, units <= 64.  The backward reads the forward's workspace (same pointer, untouched
 * in between) and returns the gradients of inputs (may be NULL), weight (units,cin), bias, gamma, beta. */
size_t vn_vfe_layer_workspace_bytes(int64_t K, int32_t T, int32_t cin, int32_t units);
int vn_vfe_layer_fwd(const float *inputs /*[K,T,cin]*/, const uint8_t *mask /*[K,T]*/, int64_t K, int32_t T,
                     int32_t cin, int32_t units, const float *weight, const float *bias, const float *gamma,
                     const float *beta, float *running_mean, float *running_var, int32_t training, float momentum,
                     float eps, float *out /*[K,T,2*units]*/, void *workspace, size_t workspace_bytes, vnStream stream);
int vn_vfe_layer_bwd(const float *inputs, const uint8_t *mask, const float *d_out /*[K,T,2*units]*/, int64_t K,
                     int32_t T, int32_t cin, int32_t units, const float *weight, int32_t training, float *d_inputs,
                     float *d_weight, float *d_bias, float *d_gamma, float *d_beta, void *workspace,
                     size_t workspace_bytes, vnStream stream);

/* ------------------------------------------------------------------------
 * Sparse -> dense scatter — model.py:102-106 (sparse COO .to_dense()).
 * dense[b,z,y,x,:] = voxelwise[k,:]; zero elsewhere.  Coordinates unique.
 * dense is f32 (B,D,H,W,C), bf16, or (split != 0) bf16 [hi|lo] with dense_channels = 2C.
 * Backward = row gather.  Deterministic.
 * ---------------------------------------------------------------------- */
int vn_scatter_dense_fwd(const float *voxelwise /*[K,C]*/, const int64_t *coord /*[K,4]*/,
                         int64_t K, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W,
                         void *dense, vnDtype dense_dtype, int32_t dense_channels,
                         int32_t split, vnStream stream);
/* The same scatter WITHOUT the zero fill, for a dense buffer the caller keeps all-zero between steps: writes the K
 * voxel rows, or — voxelwise == NULL — zeros at those rows (undoing the previous call).  A persistent grid then costs
 * 2 x K rows of writes per step instead of a 721 MB fill. */
int vn_scatter_dense_update(const float *voxelwise /* (K,C) or NULL */, const int64_t *coord, int64_t K,
                            int32_t C, int32_t B, int32_t D, int32_t H, int32_t W, void *dense,
                            vnDtype dense_dtype, int32_t dense_channels, int32_t split, vnStream stream);

int vn_scatter_dense_bwd(const void *d_dense, vnDtype dtype, const int64_t *coord,
                         int64_t K, int32_t C, int32_t B, int32_t D, int32_t H, int32_t W,
                         float *d_voxelwise /*[K,C]*/, vnStream stream);

/* ------------------------------------------------------------------------
 * Convolutions — model.py:111-199 (ConvMD: Conv2d/Conv3d; DeConv2d:
 * ConvTranspose2d) as ONE gather-GEMM on the matrix cores.
 *
 *   out[m, n] = bias[n] + sum_{tap, k} src[site(m, tap), k] * w[tap][n][k]
 *
 * m runs over the "row" sites (B, Dr, Hr, Wr); site(m, tap) is, per axis,
 *   s = (row * mul + tap * tmul - pad) / div   (valid iff divisible, 0 <= s < S)
 * and an invalid site contributes zero.  Forward conv (mul = stride, tmul = 1,
 * div = 1), the data-gradient of a strided conv and ConvTranspose2d forward
 * (mul = 1, tmul = -1, pad = -p, div = stride), and the data-gradient of a
 * ConvTranspose2d are all instances; the host code picks the geometry and the
 * packed weight orientation.  div > 1 is executed as div^3 (div^2) residue
 * classes of a stride-1 gather, all inside one launch.
 *
 * Operands are bf16 with fp32 accumulation on v_mfma_f32_16x16x32_bf16.
 * (The "split" bf16x3 mode of rounds 1-4 — [hi | lo] 2C-wide rows, weights [hi ; hi ; lo], src_wrap = 2C — was retired in
 * round 5: vnConv.src_wrap, the `split` argument of the weight-gradient entry points and vn_pack_weight's split3 must be 0
 * (VN_EUNSUPPORTED otherwise).  The fp32-accurate products are VN_F32X3 / VN_F32X3S: same error, one launch.)
 * Addresses are explicit strides in ELEMENTS, so channel slices of a wider
 * buffer (the 768-channel concat, model.py:271-273) and the BEV fold
 * (model.py:262) are views, not copies.
 * ---------------------------------------------------------------------- */
typedef struct {
    int32_t dtype;        /* operand type of src / w_packed (/ rows in wgrad): VN_BF16, or VN_F32 =
                             exact fp32 products on v_mfma_f32_16x16x4_f32 (1/16 of the bf16 rate) */
    int32_t B;
    int32_t Ds, Hs, Ws;   /* source (gathered) tensor sites */
    int32_t Dr, Hr, Wr;   /* row (produced) tensor sites */
    int32_t Cs;           /* GEMM K per tap (multiple of 8 bf16 / 4 fp32 elements; 3C in split mode) */
    int32_t src_wrap;     /* must be 0 (the K wrap of the retired bf16x3 mode) */
    int32_t Cr;           /* GEMM N = row channels (multiple of 4) */
    int32_t kD, kH, kW;   /* taps */
    int32_t mulD, mulH, mulW;
    int32_t tmulD, tmulH, tmulW;
    int32_t padD, padH, padW;
    int32_t divD, divH, divW;
    int64_t src_sB, src_sD, src_sH, src_sW; /* source strides, elements */
    int64_t out_sB, out_sD, out_sH, out_sW; /* row/output strides, elements */
} vnConv;

/* stats_slab: NULL, or float[vn_conv_stats_slab_rows(geom)][2][Cr]: every workgroup
 * writes the per-channel sum / sum of squares of (out - bias) over its valid rows
 * (plain stores, deterministic) — the train-mode BatchNorm reduction fused into the
 * epilogue; vn_bn_finalize_slab reduces it.  Only for div == 1 geometries. */
int64_t vn_conv_stats_slab_rows(const vnConv *geom);
int vn_conv_gather_gemm(const void *src, const void *w_packed /*[taps][Cr][Cs]*/,
                        const float *bias /*[Cr] or NULL*/, void *out, vnDtype out_dtype,
                        const vnConv *geom, int32_t accumulate, float *stats_slab,
                        vnStream stream);
/* Introspection for the parity tests (no launch): which kernel / tile vn_conv_gather_gemm picks for `geom`:
 * 100 + k_conv_patch tile id (0 = 10x16, 1 = 8x32, 2 = 4x16, 3 = 6x32, 4 = 6x16, 5 = 8x16 pixels), else the
 * k_gather_gemm tile id (0 = 256x64, 1 = 128x128, 2 = 64x128, 3 = 64x64, 4 = 160x128 rows x channels); < 0: bad geom. */
int32_t vn_conv_plan_id(const vnConv *geom);

/* Weight-gradient: dw[tap][n][k] += sum_m src[site(m,tap), k] * rows[m, n]
 * fp32, packed [taps][Cr][C] orientation, C = real source channels — the caller zeroes dw first.
 * The sum over m is split into row chunks whose partial tiles go to `workspace`
 * (vn_conv_wgrad_workspace_bytes; n_rows = 0 for the dense form) and are then added in a fixed order: no
 * atomics, bit-reproducible.  A NULL / smaller workspace only means fewer chunks (less parallelism).
 * rows_* strides address the (B,Dr,Hr,Wr,Cr) gradient.  split must be 0 (retired, see above).
 * geom->dtype VN_F32X3S: BOTH operands are stored split; VN_F32X3: both are fp32 and split in registers. */
size_t vn_conv_wgrad_workspace_bytes(const vnConv *geom, int32_t split, int64_t n_rows);
int vn_conv_wgrad(const void *src /*bf16*/, const void *rows /*bf16*/, float *dw_packed,
                  const vnConv *geom, int32_t split, void *workspace, size_t workspace_bytes,
                  vnStream stream);
/* Introspection (no launch): 200 = k_wgrad_patch, else 1000 * three-tap + 10 * TN + TK of k_wgrad<TN,TK> (tile =
 * 32 TN x 32 TK channels) for this geometry. */
int32_t vn_conv_wgrad_plan_id(const vnConv *geom, int32_t split, int64_t n_rows);
/* Same products, but the row-chunk partials are left in the workspace: chunk c at workspace + c * (taps*Cr*C) floats,
 * *chunks (host) = their number.  vn_unpack_wgrads_batch sums them (vnUnpackJob.chunks) while it converts the layout,
 * so a backward pass needs no per-layer reduction launch and no zeroed accumulator.  row_list != NULL: the
 * row-list form (vn_conv_wgrad_rows' operands).  The workspace must hold vn_conv_wgrad_workspace_bytes. */
int vn_conv_wgrad_partials(const void *src, const void *rows, const vnConv *geom, int32_t split,
                           const int64_t *row_list, int64_t n_rows, void *workspace,
                           size_t workspace_bytes, int32_t *chunks, vnStream stream);
/* One of the three bf16 products of an fp32x3 weight gradient over operands in split storage (geom->dtype VN_F32X3S):
 * pass 0 = hi(src).hi(rows), 1 = lo(src).hi(rows), 2 = hi(src).lo(rows) on the bf16 nine-tap patch kernel, reading the
 * halves in place.  Only the geometries of that kernel (the 64-channel Conv3d layers, model.py:207-209), else
 * VN_EUNSUPPORTED.  Lay the three passes' partial slabs one after the other; the unpack sums them like row chunks. */
int vn_conv_wgrad_partials_split_pass(const void *src, const void *rows, const vnConv *geom, int32_t pass, void *workspace,
                                      size_t workspace_bytes, int32_t *chunks, vnStream stream);

/* A data-gradient launch (ConvMD backward, model.py:111-167) that also leaves the BatchNorm-backward sums of the layer
 * BELOW in its epilogue: out = the gradient w.r.t. that layer's activation a = relu(BN(y)); bn_y = that layer's conv
 * output (same site strides as out), bn_stats its forward statistics [4][Cr] (vn_bn_finalize_slab);
 * slab[vn_conv_stats_slab_rows(geom)][2][Cr] receives per workgroup sum dz and sum dz*xhat, the rows
 * vn_bn_bwd_finalize_slab reads — the vn_bn_bwd_reduce_slab launch is saved.  Only the geometries with
 * vn_conv_plan_id == 123 (small-image 3x3 kernel); VN_EUNSUPPORTED otherwise. */
int vn_conv_dgrad_bn_bwd(const void *src, const void *w_packed, void *out, vnDtype out_dtype, const vnConv *geom,
                         const void *bn_y, vnDtype bn_y_dtype, const float *bn_stats, float *slab, vnStream stream);
/* Row-list ("sparse rows") variants for the first middle layer, whose input grid is ~99 % empty:
 * the produced rows are an explicit list of (b,d,h,w) int64 coordinates instead of the dense
 * (B,Dr,Hr,Wr) grid.  row_count (device int32, may be NULL = row_cap) lets the launch be sized by a
 * capacity known on the host while the true count stays on the device.  out_linear != 0: output row i is
 * written at out + i*out_sW (e.g. the (K,128) voxel gradient); else at the site given by the coordinates.
 * Any div (strided transposed gather) is allowed.  In vn_conv_wgrad_rows the rows operand is the
 * [n_rows][Cr] matrix of the list rows (stride out_sW) and dw is [taps][Cr][Cs]. */
int vn_conv_gather_gemm_rows(const void *src, const void *w_packed, const float *bias, void *out,
                             vnDtype out_dtype, const vnConv *geom, const int64_t *row_list,
                             int64_t row_cap, const int32_t *row_count, int32_t out_linear,
                             float *stats_slab, vnStream stream);
int vn_conv_wgrad_rows(const void *src, const void *rows, float *dw_packed, const vnConv *geom,
                       const int64_t *row_list, int64_t n_rows, void *workspace, size_t workspace_bytes,
                       vnStream stream);
/* vn_conv_wgrad_partials over a row list whose length is only known on the device: row_cap = the list's capacity (it
 * sizes the launch and the chunking), *row_count (device) the valid rows; chunks past the count store zero partials. */
int vn_conv_wgrad_partials_counted(const void *src, const void *rows, const vnConv *geom, const int64_t *row_list,
                                   int64_t row_cap, const int32_t *row_count, void *workspace, size_t workspace_bytes,
                                   int32_t *chunks, vnStream stream);
/* Active output sites of a forward conv over a sparse input: the ordered (b,d,h,w) list of the sites
 * whose receptive field contains at least one of the K occupied voxel coordinates (coord (K,4) int64
 * [b,z,y,x]).  geom = the conv's forward geometry.  list holds up to cap rows; *count = min(n, cap).
 * Deterministic order (ascending linear site index). */
size_t vn_active_sites_workspace_bytes(const vnConv *geom);
int vn_active_sites(const int64_t *coord, int64_t K, const vnConv *geom, void *workspace,
                    size_t workspace_bytes, int64_t *list, int64_t cap, int32_t *count, vnStream stream);
/* "Rulebook" evaluation of a conv over a sparse input (the first middle layer, model.py:207 over model.py:102-106),
 * in three calls: (1) vn_voxel_index_grid: int32 grid over the INPUT cells, voxel row index or -1;
 * (2) P[v][t][:] = W[t] . x[v] for every voxel and tap = ONE dense vn_conv_gather_gemm of the (K,Cin) voxel rows
 * against the packed [taps*Cout][Cin] weights (fp32 output, row stride taps*Cout); (3) vn_rulebook_combine: every
 * listed (active) output site adds the P rows of the taps whose source cell is occupied, in tap order, + bias ->
 * y at the site (dense addressing) and, optionally, per-workgroup sum / sum of squares (stats_slab
 * [vn_rulebook_slab_rows(cap)][2][Cout], the layout vn_bn_finalize_slab reads).  Work ~ K*taps instead of sites*taps.  Cout must be 64. */
int vn_voxel_index_grid(const int64_t *coord, int64_t K, int32_t B, int32_t D, int32_t H, int32_t W,
                        int32_t *grid /* (B,D,H,W) */, vnStream stream);
int64_t vn_rulebook_slab_rows(int64_t cap);   /* rows of vn_rulebook_combine's stats_slab for a list capacity */
int vn_rulebook_combine(const float *P, const int32_t *index_grid, const int64_t *list, int64_t cap,
                        const int32_t *count, const vnConv *geom, const float *bias, void *y,
                        vnDtype y_dtype, float *stats_slab, vnStream stream);
/* y[m][0:C] = values[0:C] for M rows (the conv output at inactive sites is the bias) */
int vn_fill_rows(void *y, vnDtype dtype, int64_t M, int32_t C, int64_t stride, const float *values,
                 vnStream stream);

/* Packing between torch parameter layouts and the kernels' [taps][N][K] bf16.
 * mode 0: Conv weight (Cout,Cin,k...) -> forward operand   [tap][Cout][Cin]
 * mode 1: Conv weight                 -> data-grad operand [tap][Cin][Cout]
 * mode 2: ConvTranspose weight (Cin,Cout,kh,kw) -> forward operand [tap][Cout][Cin]
 * mode 3: ConvTranspose weight        -> data-grad operand [tap][Cin][Cout]
 * split3: must be 0 (the [hi;hi;lo] K expansion of the retired bf16x3 mode).
 * packed_dtype VN_F32X3 (operand of a convolution launched with vnConv.dtype VN_F32X3): rows of K fp32-sized slots
 * in the "split fp32" format of VN_F32X3S: every aligned group of 8 input channels (32 B) = the eight hi bf16 parts, then
 * the eight lo parts (hi = bf16(w), lo = bf16(w - hi)) — a lane of the kernels reads the group 8 fq .. 8 fq + 7 of each
 * 128-B chunk as its eight k values.  Needs K % 32 == 0; for other K the packed operand is plain fp32 and the kernels split
 * it in registers (the same values either way).
 * cin_fold f: the packed Cin index p stands for torch channel (p % (Cin/f))*f + p/(Cin/f)
 * (f = 2 implements the BEV reshape of model.py:262, channel = c*2 + d; else 1). */
int vn_pack_weight(const float *w, int32_t c_out, int32_t c_in, int32_t taps, int32_t mode,
                   int32_t split3, int32_t cin_fold, void *packed, vnDtype packed_dtype,
                   vnStream stream);
/* inverse for gradients: packed fp32 [tap][N][K] (mode 0 or 2 orientation) -> torch layout */
int vn_unpack_wgrad(const float *dw_packed, int32_t c_out, int32_t c_in, int32_t taps,
                    int32_t mode, int32_t cin_fold, float *dw, vnStream stream);
/* Batched forms of the two calls above: all layers of a step in one launch (the single-layer launches are a few
 * microseconds of dispatch each, 72 per train step).  Fields as the arguments of vn_pack_weight / vn_unpack_wgrad. */
typedef struct vnPackJob {
    const float *w;
    void *packed;
    int32_t c_out, c_in, taps, mode, split3, cin_fold;
    int32_t packed_dtype;   /* vnDtype */
    int32_t pad_;
} vnPackJob;
typedef struct vnUnpackJob {
    const float *dw_packed;
    float *dw;
    int32_t c_out, c_in, taps, mode, cin_fold;
    int32_t chunks;          /* > 1: dw = sum over c < chunks (in order) of dw_packed[c * chunk_stride + i] */
    int64_t chunk_stride;    /* elements; the chunk partials of vn_conv_wgrad_partials */
} vnUnpackJob;
int vn_pack_weights_batch(const vnPackJob *jobs /* host array */, int32_t n, vnStream stream);
int vn_unpack_wgrads_batch(const vnUnpackJob *jobs /* host array */, int32_t n, vnStream stream);


/* ------------------------------------------------------------------------
 * Camera field-of-view crop of a raw Velodyne sweep — voxelnet/preprocess_data.py:42-103 (prepare_velo_points,
 * project_velo_to_img and the in-image test of align_img_and_velo; main() rewrites the .bin files with the survivors,
 * :151-154), SURVEY.md 8(f)-3.  points (n,4) fp32 [x,y,z,reflectance] on the device; P_3x4 / Tr_velo_to_cam_4x4 /
 * R_rect_4x4: HOST pointers to the float32 matrices load_calib returns (row-major).  A point survives when reflectance
 * > 0, its rectified camera z >= 0 and its rounded pixel satisfies 0 < col < image_cols, 0 < row < image_rows (float32
 * arithmetic, np.round = round half to even).  out_points (capacity n rows) receives the survivors in input order,
 * out_index (n int32, may be NULL) their input row numbers, *out_count (device int32) their number; rows
 * [*out_count, n) of out_points are filled with NaN points, which every range test drops (vn_voxelize_index on all n
 * rows gives the result of the first *out_count rows bit for bit), so the input pipeline never reads the count back.
 * Asynchronous.
 * ---------------------------------------------------------------------- */
size_t vn_fov_crop_workspace_bytes(int64_t n);
int vn_fov_crop(const float *points, int64_t n, const float *P_3x4, const float *Tr_velo_to_cam_4x4,
                const float *R_rect_4x4, int32_t image_rows, int32_t image_cols, float *out_points,
                int32_t *out_index, int32_t *out_count, void *workspace, size_t workspace_bytes, vnStream stream);

/* ------------------------------------------------------------------------
 * Point-cloud augmentation — the per-point half of pcl_augmentation (voxelnet/dataset.py:122-219; the moves are
 * point_transform, dataset.py:264): the stage between the field-of-view crop and the voxelizer (csrc/augment.hip).  The
 * random draw, the collision test (calc_iou2d, :222-240) and the moved labels are O(boxes) host work
 * (voxelnet_amd/augment.py).  points / out: (n,4) fp32 [x,y,z,reflectance], 16-byte aligned; out may BE points (in
 * place) and must not overlap it otherwise.  Reflectance is copied.
 *   rigid motion (translate, then the ROW vector times the z-rotation: a rotation by -rz about the lidar origin), in
 *   float64 exactly as written, no contraction, rounded once to fp32:
 *     X = x + tx, Y = y + ty, Z = z + tz;   x' = X*c + Y*s,   y' = -(X*s) + Y*c,   z' = Z
 *   VN_AUGMENT_BOXES : boxes = DEVICE table of n_boxes <= VN_AUGMENT_MAX_BOXES entries (16-byte aligned).  A point
 *                      walks the table in index order on its CURRENT value and is moved by every entry whose bounds
 *                      hold it (lo <= p <= hi on the three axes, fp32, inclusive) — the reference's in-place loop.
 *                      c, s, scale are ignored.  n_boxes == 0: a copy (nothing at all when out == points).
 *   VN_AUGMENT_ROTATE: the motion with t = 0 and the HOST's c = cos(angle), s = sin(angle) for every point.
 *   VN_AUGMENT_SCALE : x, y, z each multiplied by scale in fp32.
 * A NaN point (the padding rows of vn_fov_crop) fails every bounds test and stays NaN in the other two modes.
 * n == 0 is a no-op.  Asynchronous; no workspace.
 * ---------------------------------------------------------------------- */
#define VN_AUGMENT_MAX_BOXES 128
#define VN_AUGMENT_BOXES 0
#define VN_AUGMENT_ROTATE 1
#define VN_AUGMENT_SCALE 2
typedef struct vnAugmentBox {
    float lo[3], hi[3];   /* x, y, z bounds of the UNMOVED box: axis-aligned hull of its eight corners */
    double tx, ty, tz;    /* translation, applied first */
    double c, s;          /* cos(rz), sin(rz) */
} vnAugmentBox;           /* 64 bytes */
int vn_augment_points(const float *points, int64_t n, int32_t mode, const vnAugmentBox *boxes, int32_t n_boxes, double c,
                      double s, float scale, float *out, vnStream stream);

/* The composed recipe (SECOND / PointPillars: per-object noise, flip, global rotation, scaling, translation) in ONE
 * launch — vn_augment_compose, beside the three modes above (csrc/augment.hip; the draw is voxelnet_amd/augment.py's
 * draw_compose).  points / out as above (out may BE points); moves = DEVICE table of 0 <= n_moves <=
 * VN_AUGMENT_MAX_BOXES entries, 16-byte aligned; affine = HOST pointer, read at call time.  Per point, widened exactly to
 * float64, evaluated as written without contraction, rounded once to fp32; every cos / sin is the host's:
 *   membership  the test of vn_points_in_boxes on the ORIGINAL point and the UNMOVED box:
 *                 dx = px - x; dy = py - y; u = dx*c + dy*s; v = -(dx*s) + dy*c
 *                 inside <=> |u| <= hl and |v| <= hw and z0 <= pz <= z1                      (inclusive)
 *               the lowest entry that holds the point wins; a point takes AT MOST ONE object move
 *   object move X = (x + tx) + (dx*rc - dy*rs);  Y = (y + ty) + (dx*rs + dy*rc);  Z = pz + tz
 *               (the point turns about ITS box's centre, then travels with it); in no box: X, Y, Z = px, py, pz
 *   affine      x' = (a00*X + a01*Y) + bx;  y' = (a10*X + a11*Y) + by;  z' = sz*Z + bz      for every point
 * Reflectance is copied.  A NaN coordinate fails the membership test and stays NaN through the affine.
 * VN_EINVAL: n outside [0, 2^31), n_moves outside [0, VN_AUGMENT_MAX_BOXES], affine NULL, moves NULL with n_moves > 0,
 * points or out NULL with n > 0; VN_EUNSUPPORTED: a misaligned pointer.  n == 0 is a no-op.  Asynchronous; no workspace. */
typedef struct vnObjectMove {
    double x, y, z0, z1, hl, hw, c, s;   /* the UNMOVED box: vnGtBox's fields (below) and its inside test */
    double tx, ty, tz;                   /* translation of the object */
    double rc, rs;                       /* cos / sin of the object's turn about ITS centre */
    double pad[3];
} vnObjectMove;                          /* 128 bytes */
typedef struct vnAffine {
    double a00, a01, a10, a11;           /* the x / y part */
    double sz;                           /* z scale */
    double bx, by, bz;                   /* translation, applied last */
} vnAffine;                              /* 64 bytes */
int vn_augment_compose(const float *points, int64_t n, const vnObjectMove *moves, int32_t n_moves, const vnAffine *affine,
                       float *out, vnStream stream);

/* ------------------------------------------------------------------------
 * Ground-truth database sampling ("GT-paste") — the per-point half (csrc/gtsample.hip): cut labelled objects with their
 * points out of the training frames, paste a few into every training frame where they collide with nothing.  The
 * reference has no counterpart; the draw and the collision test are O(boxes) host work (voxelnet_amd/gtsample.py).
 * points (n,4) fp32 [x,y,z,reflectance], 16-byte aligned; boxes = DEVICE table of 0 <= n_boxes <= VN_GT_MAX_BOXES
 * entries (16-byte aligned).  An entry comes from a lidar box (x, y, z, h, w, l, r): z0 = z, z1 = z + h, hl = l / 2,
 * hw = w / 2, c = cos(r), s = sin(r) — the HOST's cos / sin.
 *   inside, for a point (px, py, pz) widened exactly to float64, in float64 exactly as written, no contraction:
 *     dx = px - x;  dy = py - y;  u = dx*c + dy*s;  v = -(dx*s) + dy*c
 *     inside  <=>  |u| <= hl  and  |v| <= hw  and  pz >= z0  and  pz <= z1      (inclusive; a NaN anywhere fails)
 *   There is no fp32 prefilter: every decision is the float64 one.
 * vn_points_in_boxes: out_index[i] (n int32) = the lowest table index whose box holds point i, else -1; out_counts[j]
 *   (n_boxes int32, may be NULL) = the number of points inside box j — a point inside two boxes counts for both; integer
 *   adds only, so the counts are deterministic.  n == 0 is a no-op apart from the zeroed counts.  No workspace.
 * vn_gt_paste: a scene row is kept when none of its x, y, z is NaN (the padding rows of vn_fov_crop go) and it is inside
 *   no box.  out_points (cap rows, cap >= n + m, else VN_EINVAL): rows [0, k) = the kept scene rows in input order,
 *   reflectance copied; rows [k, k + m) = obj_points (m,4) in order, verbatim; rows [k + m, cap) = NaN points, which every
 *   range test downstream drops, so the voxelizer runs on all cap rows without the count being read back; *out_count
 *   (device int32) = k + m.  out_points must not overlap either input (VN_EINVAL).  n, m and n_boxes may each be 0.
 *   Misaligned pointers: VN_EUNSUPPORTED; a workspace below vn_gt_paste_workspace_bytes(n): VN_EWORKSPACE.
 *   Three launches (flags + per-workgroup counts, one-workgroup scan, compaction + append + NaN fill); no workgroup
 *   waits on another one.
 * Asynchronous.
 * ---------------------------------------------------------------------- */
#define VN_GT_MAX_BOXES 128
typedef struct vnGtBox {
    double x, y;          /* footprint centre */
    double z0, z1;        /* bottom and top: z, z + h */
    double hl, hw;        /* half length (along the heading), half width */
    double c, s;          /* cos(r), sin(r) */
} vnGtBox;                /* 64 bytes */
int vn_points_in_boxes(const float *points, int64_t n, const vnGtBox *boxes, int32_t n_boxes, int32_t *out_index,
                       int32_t *out_counts, vnStream stream);
size_t vn_gt_paste_workspace_bytes(int64_t n);
int vn_gt_paste(const float *points, int64_t n, const vnGtBox *boxes, int32_t n_boxes, const float *obj_points, int64_t m,
                float *out_points, int64_t cap, int32_t *out_count, void *workspace, size_t workspace_bytes,
                vnStream stream);

/* ------------------------------------------------------------------------
 * The occlusion-consistent paste (csrc/gtsample.hip): vn_gt_paste with a coarse range image
 * of the frame.  A pasted object whose points are mostly hidden behind scene points is rejected; the hidden points of an
 * accepted object go; scene points, and points of other pasted objects, in the shadow of an accepted object go.
 * Everything below is float64, evaluated as written, no contraction, IEEE divides.
 *   Bin of a point (px, py, pz), float32 widened exactly — four side faces of a cube around the sensor:
 *     ax = |px|, ay = |py|;  ax >= ay: a = ax, face = px > 0 ? 0 : 2, u = py / a;  else: a = ay, face = py > 0 ? 1 : 3,
 *     u = px / a;  v = pz / a.  No bin when any of x, y, z is non-finite or a == 0.
 *     iu = min(floor((u + 1.0) * (nu / 2)), nu - 1);  iv = floor((v - v_lo) * v_scale), iv < 0 or iv >= nv: no bin.
 *     bin = (face * nv + iv) * nu + iu;  depth = a (exactly a float32: its bit pattern as uint32 orders like the value).
 *   vnVisGrid (HOST struct): nu even in 2..2048, nv in 1..256, v_lo < v_hi finite, v_scale = nv / (v_hi - v_lo) computed
 *     by the caller (finite, > 0), margin >= 0 (+inf allowed, NaN refused), min_visible >= 0.
 *   obj_offsets: HOST pointer to n_boxes + 1 int32, non-decreasing, [0] == 0, [n_boxes] == m, read and validated during
 *     the call; object o owns object rows [offsets[o], offsets[o+1]).
 *   1. Dscene[bin] = min depth over the scene rows with no NaN in x, y, z that have a bin and lie inside NO box of the
 *      table (vn_gt_paste's inside test).
 *   2. an object point is visible <=> none of x, y, z is NaN and not (it has a bin and (double)depth >
 *      (double)Dscene[bin] + margin);  visible[o] = the visible points of object o;  accepted[o] <=> visible[o] >= min_visible.
 *   3. Dobj[bin] = min, over the visible points of accepted objects that have a bin, of (depth bits << 32) | o: the
 *      nearest depth and its owner, equal depths to the lower object.
 *   4. a scene row is kept <=> no NaN in x, y, z, inside no ACCEPTED box, and not (it has a bin, the bin has an owner and
 *      depth > Dobj.depth + margin);  an object point is kept <=> visible, its object accepted, and not (it has a bin
 *      whose owner is ANOTHER object and depth > Dobj.depth + margin).
 *   5. out_points (cap rows, cap >= n + m, else VN_EINVAL): rows [0, k) = the kept scene rows in input order, [k, k + m')
 *      = the kept object points in input order, verbatim, [k + m', cap) = NaN points;  *out_count = k + m'.
 *   6. out_visible[n_boxes] (pass 2's counts: the caller derives acceptance from them), out_kept[n_boxes] (the final
 *      points per object), out_stats[2] = {scene rows removed by an accepted box, scene rows removed by shadow only}:
 *      DEVICE int32, 4-byte aligned; out_visible / out_kept may be NULL when n_boxes == 0.
 *   Acceptance is decided by scene visibility only: an accepted object may end with fewer than min_visible points after
 *   another pasted object culls it.  Scene points inside a REJECTED object's box stay, but were no occluders in pass 1.
 *   margin = +inf with min_visible = 0 is vn_gt_paste bit for bit (for object points without NaN coordinates).
 * Bad sizes, a bad grid, bad offsets, overlapping out_points / inputs: VN_EINVAL; a workspace below
 * vn_gt_paste_visible_workspace_bytes(n, m, grid) (0 for bad arguments): VN_EWORKSPACE; pointers (workspace included) off
 * their 16-byte / 4-byte alignment: VN_EUNSUPPORTED — all decided before the first launch.  The depth buffers live in the
 * workspace and are reset on the stream by every call.  Seven launches (reset, scene depth, visible counts, object depth,
 * keep flags over the n + m rows, the one-workgroup scan, compaction + NaN fill); integer minima and sums only, so the
 * result does not depend on the order of the atomics; no workgroup waits on another one.  Asynchronous.
 * ---------------------------------------------------------------------- */
typedef struct vnVisGrid {
    int32_t nu, nv;             /* bins across a face, rows */
    double v_lo, v_hi;          /* the rows cover v = z / a in [v_lo, v_hi) */
    double v_scale;             /* nv / (v_hi - v_lo) */
    double margin;              /* metres of depth a point may lie behind the front of its bin */
    int32_t min_visible;        /* an object needs this many visible points */
    int32_t reserved;
} vnVisGrid;                    /* 48 bytes */
size_t vn_gt_paste_visible_workspace_bytes(int64_t n, int64_t m, const vnVisGrid *grid);
int vn_gt_paste_visible(const float *points, int64_t n, const vnGtBox *boxes, int32_t n_boxes, const float *obj_points,
                        int64_t m, const int32_t *obj_offsets, const vnVisGrid *grid, float *out_points, int64_t cap,
                        int32_t *out_count, int32_t *out_visible, int32_t *out_kept, int32_t *out_stats, void *workspace,
                        size_t workspace_bytes, vnStream stream);

/* ------------------------------------------------------------------------
 * Point shuffle on the device — the reference's np.random.shuffle(point_cloud) in front of the voxelizer
 * (voxelnet/utils.py:35), which decides which <= T points of a crowded voxel survive, as a row gather right behind the
 * host->device copy (csrc/shuffle.hip; the draws are voxelnet_amd/shuffle.py).  points / out: (n,4) fp32
 * [x,y,z,reflectance], 16-byte aligned.  In both calls output row i is a BIT copy of input row p(i), moved as one 16-byte
 * word: NaN payloads, -0.0 and the reflectance survive.
 *   vn_permute_points: p(i) = index[i]; index = DEVICE table of n int32.  With the table np.random.shuffle made of
 *     arange(n) — the same Mersenne-Twister draws as the shuffle of the (n,C) cloud itself — out is the reference's
 *     shuffled cloud bit for bit.  An index outside [0, n) writes a NaN point (four 0x7FC00000 words) to that row and
 *     reads nothing: no table makes the kernel read outside points.
 *   vn_shuffle_points: p = a keyed bijection of [0, n), evaluated per thread; keys = SIX uint32 in HOST memory, read during
 *     the call and passed to the kernel by value.  A six-round Feistel network over 2h bits, walked until it lands inside
 *     the range; exact uint32 arithmetic (wrapping multiplies):
 *       k = max(2, bit_length(n - 1));   h = (k + 1) / 2;   mask = 2^h - 1        (n < 2^31, so 2h <= 32)
 *       fmix32(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
 *       F(x):  L = x >> h;  R = x & mask;  for r in 0..5:  (L, R) = (R, L ^ (fmix32(R ^ keys[r]) & mask));  (L << h) | R
 *       p(i):  x = F(i);  while x >= n: x = F(x)
 *     F is a bijection of [0, 2^2h) and i lies on its own cycle, so the walk ends; 2^2h < 4n.
 * A null pointer with n > 0, n < 0 or n > 2^31 - 1: VN_EINVAL.  out overlapping points (a gather cannot run in place) or
 * the index table: VN_EINVAL.  Misaligned pointers: VN_EUNSUPPORTED.  n == 0 is a no-op.  Every argument is checked
 * before anything is launched.  One launch each, one thread per output row; asynchronous; no workspace.
 * ---------------------------------------------------------------------- */
int vn_permute_points(const float *points, int64_t n, const int32_t *index, float *out, vnStream stream);
int vn_shuffle_points(const float *points, int64_t n, const uint32_t keys[6], float *out, vnStream stream);

/* ------------------------------------------------------------------------
 * Part-aware object augmentation (csrc/part_augment.hip; SE-SSD's "shape-aware", PA-AUG's
 * "part-aware" augmentation): an object's box is cut into the six pyramids that join its centre to its faces; per object
 * one pyramid may lose all its points (drop), one may be thinned (thin), one may be exchanged with the same pyramid of
 * another object, rescaled to that object's box (swap).  The draw is O(boxes) host work (voxelnet_amd/part_augment.py);
 * this is the per-point half, between the paste and the augmentation.  points / out: (n,4) fp32 [x,y,z,reflectance],
 * 16-byte aligned; boxes = DEVICE table of 0 <= n_boxes <= VN_PART_MAX_BOXES entries, 16-byte aligned; gate = DEVICE
 * int32 (n_boxes - gate_first values) or NULL.  Every decision widens float32 exactly to float64 and is evaluated as
 * written, no contraction; the kernels hold no divide (the ratios ru, rv, rw are the host's).
 *   live     entry o is DEAD when gate != NULL and o >= gate_first and gate[o - gate_first] < gate_min (with the visible
 *            counts of vn_gt_paste_visible as the gate: the objects that paste rejected).  A dead entry holds no point, its
 *            counts and stats are zero, and a swap whose partner is dead is void.
 *   owner    a row with a NaN in x, y or z has no owner; otherwise the LOWEST live entry whose box holds the point
 *            (vnGtBox's inside test, inclusive).  A row without an owner is a BIT copy of the input row (one 16-byte word).
 *   pyramid  of an owned row, with dx, dy, u, v of the inside test:
 *              hh = (z1 - z0) * 0.5;  w = pz - (z0 + hh)
 *              m0 = |u| * (hw * hh);  m1 = |v| * (hl * hh);  m2 = |w| * (hl * hw)
 *              axis = 0 when m0 >= m1 and m0 >= m2, else 1 when m1 >= m2, else 2
 *              f = 2 * axis + (that axis's coordinate (u, v, w) < 0 ? 1 : 0)
 *            (-0.0 and the box centre are face 0 of axis 0; diagonals go to the lower axis)
 *   out_counts[o][f] = the rows owned by o in pyramid f, before any operation.
 *   operations, the first that applies wins; all read the entry of the row's ORIGINAL owner o (masks are taken & 0x3F):
 *     1. drop: bit f of drop_mask -> a NaN point (four 0x7FC00000 words); out_stats[o][0]++
 *     2. thin: bit f of sparse_mask and out_counts[o][f] >= sparse_min and (fmix32((uint32)i ^ sparse_key) >> 8) >=
 *              sparse_thresh, i = the row's index in this call, fmix32 as above -> a NaN point; out_stats[o][1]++
 *     3. swap: bit f of swap_mask and p = swap_with in [0, n_boxes) and p != o and p live:
 *                u' = u * ru;  v' = v * rv;  w' = w * rw;   hh_p = (p.z1 - p.z0) * 0.5
 *                X = p.x + (u' * p.c - v' * p.s);  Y = p.y + (u' * p.s + v' * p.c);  Z = (p.z0 + hh_p) + w'
 *              each rounded once to fp32, reflectance bit-copied; out_stats[o][2]++.  A moved row takes no rule from p.
 *     otherwise the row is a bit copy.
 * No table content makes a kernel read or write outside its buffers: a swap_with outside [0, n_boxes) means no partner.
 * out may BE points (in place); otherwise it must not overlap it (VN_EINVAL).  n == 0 is a no-op apart from the zeroed
 * counts and stats; n_boxes == 0 is a copy (nothing at all when in place) and out_counts / out_stats may then be NULL.
 * VN_EINVAL: n outside [0, 2^31), n_boxes outside [0, VN_PART_MAX_BOXES], gate_first outside [0, n_boxes], a null pointer
 * with work to do; VN_EWORKSPACE: a workspace below vn_part_augment_workspace_bytes(n, n_boxes) (0 for bad arguments);
 * VN_EUNSUPPORTED: points, out, boxes or workspace off their 16-byte alignment, out_counts, out_stats or gate off their
 * 4-byte alignment — all decided before the first launch.  Three launches: zero of the counts and stats; the count
 * pass (owner + pyramid per row into the workspace as a uint16 code, a per-workgroup LDS histogram flushed with one
 * global integer add per non-empty bin); the apply pass.  No workgroup waits on another one and only integers are
 * added, so two runs give the same bits.  Asynchronous.
 * ---------------------------------------------------------------------- */
#define VN_PART_MAX_BOXES 128
typedef struct vnPartBox {
    double x, y, z0, z1, hl, hw, c, s;   /* vnGtBox's fields and its inside test */
    double ru, rv, rw;                   /* partner extent / own extent along length, width, height */
    int32_t drop_mask, sparse_mask, swap_mask;   /* bit f = pyramid f; only bits 0..5 are read */
    int32_t swap_with;                   /* partner entry, -1: none */
    uint32_t sparse_key, sparse_thresh;  /* thresh in 0 .. 2^24: a row of a thinned pyramid stays when its 24-bit hash is below it */
    int32_t sparse_min, reserved;        /* a pyramid with fewer rows is not thinned */
    double pad;
} vnPartBox;                             /* 128 bytes */
size_t vn_part_augment_workspace_bytes(int64_t n, int32_t n_boxes);
int vn_part_augment(const float *points, int64_t n, const vnPartBox *boxes, int32_t n_boxes, const int32_t *gate,
                    int32_t gate_first, int32_t gate_min, float *out, int32_t *out_counts, int32_t *out_stats,
                    void *workspace, size_t workspace_bytes, vnStream stream);

/* ------------------------------------------------------------------------
 * Native step executor — MiddleConvNet.forward (model.py:257-281) and its backward as ONE call
 * each (csrc/runtime.hip): layer table, launch geometry and workspace arena live in C++, so the
 * ~450 launches of a step cost microseconds of host time instead of a Python round trip each.
 * The workspace (vn_net_workspace_bytes, caller allocated) also keeps the activations between
 * the two calls.  mode: 0 = bf16 operands, 1 = fp32 operands (parity mode).  Layers are indexed
 * in execution order: middle_layer.0-2, block1.0-4, deconv1, block2.0-5, deconv2, block3.0-5,
 * deconv3 (23 entries); the two 1x1 heads are passed concatenated (prob rows first).
 * sparse_first: the first Conv3d runs in its row-list form (needs coord, K; backward returns
 * the (K,128) fp32 voxel gradient in d_input and needs vw_rows (K,128) in the operand dtype);
 * else d_input receives the dense (B,D,H,W,128) gradient in the operand dtype (may be NULL).
 * The backward can be issued in segments of its 24 steps (0 = heads, 1..23 = layers in backward
 * order: deconv3, block3.5..0, deconv2, block2.5..0, deconv1, block1.4..0, middle_layer.2..0) so
 * a caller can start the gradient all-reduce of finished parameter groups in between.
 * ---------------------------------------------------------------------- */
typedef struct {
    int32_t B, D, H, W;      /* dense voxel grid; D = 9 .. 12 (every depth whose three Conv3d layers fold to 2: model.py:207-209, 262) */
    int32_t block1_stride;   /* 2: Car, 1: Pedestrian/Cyclist (model.py:212-227) */
    int32_t mode;            /* 0 bf16, 1 fp32, 2 fp32x3 (fp32 storage, conv / weight-gradient products as three bf16 MFMAs: VN_F32X3) */
    int32_t training;        /* BatchNorm: batch statistics + running-stat update, or running statistics */
    int32_t sparse_first;
    int32_t prepared;        /* forward: vn_net_prepare has already been issued for this step on the same vnNet (weights packed,
                              * first layer's site list / index grid / bias fill); vn_net_forward orders itself behind it
                              * (two events: the first layer's needs, then the rest of the packing) */
    int32_t bucket_events;   /* single-call backward with a side stream: unpack each parameter group's weight gradients on the
                              * side stream at the group's end and record "group final" events (vn_net_wait_bucket);
                              * implies that the caller joins the side stream (as defer_join) */
    int32_t defer_join;      /* backward with a side stream: the last segment does NOT wait for the side stream; the
                              * weight-gradient unpack runs there and the CALLER joins it (stream wait) before anything
                              * reads the weight gradients — lets e.g. the VFE backward run beside the last weight gradients */
    int32_t grad_storage;    /* bf16 mode only: which tensors of the step are kept in fp32 instead of bf16 (bit set), DESIGN.md §4:
                              * 1 = the heads' data gradient (the 768-channel concat gradient the three deconvs' BatchNorm
                              *     backward reads), 2 = every layer's data gradient (the input of the BatchNorm backward below),
                              * 4 = every conv output y (forward), 8 = the heads' data gradient is computed from the fp32
                              * (B*S,16) logit gradient and the fp32 head weights (vn_heads_dgrad_f32) instead of their bf16
                              * roundings.  0 = everything bf16 (the shipped configuration: tools/grad_attribution.py measures
                              * that none of the four moves a gradient).  fp32 mode: 16 = diagnostic, every activation is rounded
                              * to the nearest bf16 VALUE (stored fp32; the sparse first-layer backward shortcuts are off) — the
                              * bf16 forward function with an exact fp32 backward. */
} vnNetConfig;
typedef struct {
    const float *weight, *bias, *gamma, *beta;
    float *running_mean, *running_var;
} vnLayerParams;
typedef struct {
    float *weight, *bias, *gamma, *beta;   /* overwritten */
} vnLayerGrads;
size_t vn_net_workspace_bytes(const vnNetConfig *cfg, int64_t K);
/* Read-only plan query (tests and diagnostics): where vn_net_forward leaves a layer's tensors in the workspace.  Runs the
 * same deterministic walk as vn_net_workspace_bytes; launches nothing and touches no memory.  layer: 0..22 in execution
 * order (as above); which: VN_NET_Y the conv output (pre-BatchNorm), VN_NET_A the activation, VN_NET_STATS the BatchNorm
 * statistics.  out: byte offset from the workspace base, dtype (VN_F32, VN_BF16, or VN_F32X3S for split storage: fp32x3
 * mode, layers >= 1 that are not transposed), B, D, H, W, C and element strides (the channel stride is 1).  Layouts:
 *   a of deconv3 / deconv2 / deconv1 is the channel slice at 0 / 256 / 512 of the 768-wide concatenation the heads read
 *   (C = 256, sW = 768);  a of middle_layer.2 is the BEV fold (B,1,H,W,128) with channel d*64 + c;
 *   y of middle_layer.0 with sparse_first holds values only where an occupied voxel is in reach (elsewhere it is the conv
 *   bias in the network's function, but the training forward may leave those sites unwritten; its a is complete);
 *   stats is a 4 x 256-float block whose first 4*C floats are [4][C] = mean | invstd | gamma*invstd | beta — the same
 *   vector as engine.layer_forward's (reported as W = 4 rows of C, sW = C).
 * VN_EINVAL for a null pointer, K < 0, layer or which out of range; VN_EUNSUPPORTED for a config vn_net_workspace_bytes
 * refuses. */
enum { VN_NET_Y = 0, VN_NET_A = 1, VN_NET_STATS = 2 };
typedef struct {
    int64_t offset;          /* bytes from the workspace base */
    int32_t dtype;           /* vnDtype */
    int32_t B, D, H, W, C;
    int64_t sB, sD, sH, sW;  /* element strides (4-byte elements for VN_F32X3S, as its producers count them) */
} vnNetTensorInfo;
int vn_net_tensor_info(const vnNetConfig *cfg, int64_t K, int32_t layer, int32_t which, vnNetTensorInfo *out);
/* Executor context: the HIP events of the two-stream schedule (fork / join ring, "parameter group final" events), created
 * on the current device.  Caller-owned (one per executor instance, e.g. one RPN3D module on one device) — the library
 * keeps no mutable state of its own.  Calls sharing a context must not overlap on the host. */
typedef struct vnNet vnNet;
int vn_net_create(vnNet **out);
int vn_net_destroy(vnNet *net);
/* Optional per-launch timing of the executor (bench.py's live roofline measurement, taken on the SAME native path it
 * times): after vn_net_timing_begin every launch of vn_net_prepare / vn_net_forward / vn_net_backward on this context
 * is bracketed by two HIP timing events on the stream the kernel is launched on; vn_net_timing_read stops the timing,
 * waits for the events and returns one record per launch in issue order (*count = launches recorded; at most `cap`
 * are written).  flops / bytes are the ALGORITHMIC work of the launch (2 x MACs of the layer definition
 * for forward, data gradient and weight gradient alike; tensor bytes read + written once), 0 where not defined. */
enum { VN_T_CONV_FWD = 0, VN_T_CONV_DGRAD = 1, VN_T_WGRAD = 2, VN_T_BN_APPLY = 3, VN_T_BN_BWD_REDUCE = 4,
       VN_T_BN_BWD_APPLY = 5, VN_T_BN_FINALIZE = 6, VN_T_UNPACK = 7, VN_T_PACK = 8, VN_T_FIRST = 9, VN_T_MISC = 10 };
typedef struct {
    int32_t kind;    /* VN_T_* */
    int32_t layer;   /* execution-order index 0..22, 23 = heads, -1 = all layers */
    float ms;        /* event-to-event duration of the launch */
    float start_ms;  /* start of the launch's event bracket relative to the first record of this vn_net_timing_read */
    double flops, bytes;
} vnTimingRecord;
int vn_net_timing_begin(vnNet *net, int32_t max_records);
int vn_net_timing_read(vnNet *net, vnTimingRecord *out, int32_t cap, int32_t *count);
/* Make `stream` wait until parameter group `bucket` (0: heads+deconv3+block3, 1: deconv2+block2+deconv1, 2: block1,
 * 3: middle_layer) of the most recent vn_net_backward issued with cfg->bucket_events has its final gradients. */
int vn_net_wait_bucket(vnNet *net, int32_t bucket, vnStream stream);
/* The part of the forward that does not depend on the voxel features (weight packing; sparse first layer: active
 * sites, voxel index grid, bias fill): may be issued on another stream while the VFE forward runs; then set
 * cfg->prepared for vn_net_forward.  The forward's stream need not wait for this one: vn_net_prepare records, on the
 * vnNet, one event behind what the first layer needs (issued first) and one behind the rest of the weight packing, and
 * vn_net_forward waits for the first at its start and for the second in front of the second layer.
 * cfg->prepared names the PHASE of a vn_net_prepare call: 0 = everything in one call; 1 = only the first layer's needs
 * (event 0; heads_w may be NULL) and return; 2 = only the rest (event 1), valid only right after a phase-1 call for the
 * same workspace, coord, K and grid (else VN_EINVAL) — for a caller whose heads_w is itself produced on that stream (a
 * concatenation of the two heads' parameters) and should not sit in front of the site list.  An error return clears the
 * protocol state; vn_net_forward with cfg->prepared != 0 returns VN_EINVAL unless the prepare was issued for ITS
 * workspace / coord / K / grid, and consumes it. */
int vn_net_prepare(vnNet *net, const vnNetConfig *cfg, const vnLayerParams *layers, const float *heads_w,
                   const int64_t *coord, int64_t K, void *workspace, size_t workspace_bytes, vnStream stream);
int vn_net_forward(vnNet *net, const vnNetConfig *cfg, const vnLayerParams *layers /*[23]*/,
                   const float *heads_w /*[16,768]*/, const float *heads_b /*[16]*/,
                   const void *dense, const int64_t *coord, const void *vw_rows /* (K,128) voxel rows in the operand dtype, sparse_first only */, int64_t K, void *workspace,
                   size_t workspace_bytes, float *prob /*(B,2,h,w)*/, float *reg /*(B,14,h,w)*/,
                   vnStream stream,
                   vnStream side_stream /* NULL, or a second stream deconv1 / deconv2 run on beside block2 / block3 */);
/* VN_EUNSUPPORTED when cfg->training == 0: only the train-mode BatchNorm backward exists. */
int vn_net_backward(vnNet *net, const vnNetConfig *cfg, const vnLayerParams *layers, const float *heads_w,
                    const float *d_prob, const float *d_reg, const float *prob, const void *dense,
                    const int64_t *coord, const void *vw_rows, int64_t K, void *workspace,
                    size_t workspace_bytes, const vnLayerGrads *grads /*[23]*/, float *d_heads_w,
                    float *d_heads_b, void *d_input, int32_t seg_begin, int32_t seg_end,
                    vnStream stream, vnStream side_stream /* NULL, or a second stream the weight-gradient
                    launches run on beside the data-gradient ones; joined back before the call returns */);

/* ONE call per train step (voxelnet/model.py:298-362 + voxelnet/train.py:151-154): the voxel feature encoder, the
 * middle layers + RPN, the loss, the whole backward and (n_chunks > 0) clip_grad_norm_ + SGD, issued in the order and on
 * the streams the separate calls are issued by a host that overlaps them by hand:
 *   side:  [wait stream]  counters += 1 | vn_net_prepare phase 1 | heads' parameters -> heads_w / heads_b | vn_net_prepare phase 2 |
 *          [wait targets_stream] vn_rpn_loss_norm | ... | [wait the pass] vn_rpn_loss_finalize -> loss5
 *   main:  vn_vfe_fwd (bf16 mode: vn_vfe_fwd_rows, whose last pass writes vw_rows too: no vn_cast_rows launch) |
 *          vn_net_forward | [wait the normalisers] vn_rpn_loss_spec_fwd_bwd_rows (g_loss, loss_spec): ONE launch between the heads and their
 *          backward, which also leaves the heads' gradient rows in the arena (no vn_heads_bwd launch) |
 *          vn_net_backward(0..24, defer_join) | vn_vfe_bwd | [wait side] | vn_clip_sgd
 * Same arithmetic and same results as those calls (tests/test_gpu_step.py: bit-identical); what it saves is the host's
 * work between them and four of the five loss launches on the chain between the network's forward and backward.  Every buffer is the caller's; scratch ones (voxelwise, vfe_stats, vw_rows, d_voxelwise,
 * heads_w / heads_b, d_prob / d_reg, the three workspaces) need only live until the step has run.
 * Requires cfg->sparse_first, cfg->training and a side stream (VN_EUNSUPPORTED / VN_EINVAL otherwise).
 * cfg->bucket_events is honoured (vn_net_wait_bucket after the call; pass n_chunks = 0 and update after the exchange). */
/* the loss's objective: see "RPN loss" below (vn_rpn_loss_spec_*); all zero = the reference's */
#define VN_LOSS_BCE 0
#define VN_LOSS_FOCAL 1
typedef struct {
    int32_t cls_kind;     /* VN_LOSS_BCE = 0 (reference), VN_LOSS_FOCAL = 1 */
    int32_t yaw_sin;
    float focal_alpha;
    float focal_gamma;
} vnLossSpec;
struct vnParamChunk;
typedef struct {
    const float *feature;          /* (K,T,7) */
    const int64_t *coord;          /* (K,4) */
    int64_t K;
    int32_t T;
    float bn_momentum, bn_eps;     /* the VFE's BatchNorm1d (the executor's layers use 0.1 / 1e-5 as vn_net_forward does) */
    vnVfeWeights vfe;
    vnVfeGrads vfe_grads;
    void *vfe_ws; size_t vfe_ws_bytes;            /* vn_vfe_workspace_bytes(K, T) */
    float *voxelwise;              /* (K,128) */
    float *vfe_stats;              /* 320 */
    void *vw_rows;                 /* (K,128) in the operand dtype: bf16 mode = a bf16 scratch buffer; fp32 / fp32x3 = voxelwise itself */
    float *d_voxelwise;            /* (K,128) */
    const float *prob_w, *prob_b, *reg_w, *reg_b;   /* prob_conv / reg_conv parameters: (2,768) (2) (14,768) (14) */
    float *heads_w, *heads_b;      /* scratch (16,768) (16): their concatenation, prob rows first */
    float *d_heads_w, *d_heads_b;  /* gradients of the concatenation (16,768) (16) */
    const vnLayerParams *layers;   /* [23] */
    const vnLayerGrads *grads;     /* [23] */
    void *ws; size_t ws_bytes;     /* vn_net_workspace_bytes */
    float *prob, *reg;             /* outputs (B,2,h,w) (B,14,h,w) */
    float *d_prob, *d_reg;         /* scratch, same shapes */
    const float *pos, *neg, *targets;   /* (B,h,w,2) (B,h,w,2) (B,h,w,14) */
    vnStream targets_stream;       /* NULL, or the stream those three are produced on: the loss waits for what is queued there now */
    float alpha, beta, sigma;
    void *loss_ws; size_t loss_ws_bytes;          /* vn_rpn_loss_workspace_bytes */
    float *loss5;                  /* output: loss, cls_loss, reg_loss, cls_pos_loss_rec, cls_neg_loss_rec */
    const float *g_loss;           /* device scalar: d(objective) / d(loss), normally 1 */
    const struct vnParamChunk *chunks; int32_t n_chunks;   /* vn_clip_sgd's table; n_chunks = 0: no parameter update */
    float max_norm, lr;
    int32_t scale_grads;
    void *opt_ws; size_t opt_ws_bytes;
    float *total_norm;             /* may be NULL */
    int64_t *const *bn_counters;   /* NULL, or a DEVICE array of n_bn_counters pointers: every BatchNorm's num_batches_tracked, */
    int32_t n_bn_counters;         /* += 1 each (nn.BatchNorm*.forward in train mode) — one launch on the side stream */
    vnStream stream, side_stream;
    vnLossSpec loss_spec;          /* the objective of the loss pass (vn_rpn_loss_spec_fwd_bwd_rows); all zero: the reference's */
} vnStep;
int vn_net_step(vnNet *net, const vnNetConfig *cfg, const vnStep *step);

/* ------------------------------------------------------------------------
 * Data-parallel gradient exchange over RCCL / xGMI (the reference has no distributed code):
 * thin wrappers, RCCL bound at run time (dlopen; inside a PyTorch process torch's own librccl is reused).
 * Status: VN_EUNSUPPORTED when no librccl can be found, 1000 + ncclResult_t for RCCL errors.
 * vn_comm_create is collective (every rank, on its own current device, with rank 0's 128-byte id);
 * `nccl_comm` is a plain ncclComm_t — a communicator made elsewhere (e.g. by an MPI launcher) works as well.
 * vn_allreduce_bucket: bucket[i] = sum over ranks of scale * bucket[i], in place, asynchronous on `stream`
 * (scale = 1/world: the mean stock DDP takes; scaled before the sum, so all ranks end bit-identical).
 * ---------------------------------------------------------------------- */
int vn_comm_rccl_version(void); /* ncclGetVersion() code of the librccl bound at run time (e.g. 22703), 0 if none;
                                  * every vn_comm_* / vn_allreduce_bucket call returns VN_EUNSUPPORTED unless it is 2.x:
                                  * the RCCL entry points are declared by hand (ncclUniqueId by value, ncclFloat32 = 7) */
int vn_comm_unique_id(void *id128 /* out: 128 bytes (ncclUniqueId) */);
int vn_comm_create(void **nccl_comm, const void *id128, int32_t world, int32_t rank);
int vn_comm_destroy(void *nccl_comm);
int vn_allreduce_bucket(void *nccl_comm, float *bucket, int64_t count, float scale, vnStream stream);

/* ------------------------------------------------------------------------
 * BatchNorm(+ReLU) over channels-last rows — nn.BatchNorm{1,2,3}d defaults
 * (momentum 0.1, eps 1e-5) as used at model.py:72,142,153,193.
 * Rows are M x C with `stride` elements between rows.  `fold` (1 or 2): the C
 * columns are `fold` copies of C/fold real channels (BEV view of the last
 * Conv3d, model.py:262); parameter vectors have C/fold entries, the sums /
 * stats / coef work vectors are C wide.
 * ---------------------------------------------------------------------- */
/* sums[0:C] += sum_m (y - shift), sums[C:2C] += sum_m (y - shift)^2   (double; caller zeroes)
 * shift: float[C/fold] or NULL (conditioning only; finalize takes the same shift) */
int vn_bn_stats(const void *y, vnDtype dtype, int64_t M, int32_t C, int64_t stride, int32_t fold,
                const float *shift, double *sums, vnStream stream);
/* sums -> stats[4C] = mean | invstd | S = gamma*invstd | beta  with a = S*(y-mean) + beta;
 * training: batch statistics (biased var) + running-stat update (unbiased var);
 * eval (training == 0): running statistics, sums ignored. */
int vn_bn_finalize(const double *sums, int64_t M, int32_t C, int32_t fold, const float *shift,
                   const float *gamma, const float *beta, float *running_mean, float *running_var,
                   int32_t training, float momentum, float eps, float *stats, vnStream stream);
/* same, from a vn_conv_gather_gemm stats slab: float[rows][2][C] partial sums of (y - shift) */
int vn_bn_finalize_slab(const float *slab, int64_t slab_rows, int64_t M, int32_t C, const float *shift,
                        const float *gamma, const float *beta, float *running_mean, float *running_var,
                        float momentum, float eps, float *stats, vnStream stream);
/* a = relu?(S*(y-mean) + beta) -> f32 or bf16 rows.  lo_off != 0 (split mode): the
 * bf16 residual lo = bf16(a - hi) is also written, lo_off elements after hi. */
int vn_bn_apply(const void *y, vnDtype y_dtype, int64_t y_stride, int64_t M, int32_t C,
                const float *stats, int32_t relu, void *a, vnDtype a_dtype, int64_t a_stride,
                int64_t lo_off, vnStream stream);
/* backward step 1: dz = da * (relu ? S*y+T > 0 : 1);
 * sums[0:C] += sum dz, sums[C:2C] += sum dz*xhat   (double; caller zeroes) */
int vn_bn_bwd_reduce(const void *da, vnDtype da_dtype, int64_t da_stride, const void *y,
                     vnDtype y_dtype, int64_t y_stride, int64_t M, int32_t C, const float *stats,
                     int32_t relu, double *sums, vnStream stream);
/* step 2: folds the sums; coef[3C] with dy = c0*dz + c1*(y-mean) + c2;
 * d_gamma[C/fold] = sum dz*xhat, d_beta[C/fold] = sum dz */
int vn_bn_bwd_finalize(const double *sums, int64_t M, int32_t C, int32_t fold, const float *gamma,
                       const float *stats, float *coef, float *d_gamma, float *d_beta,
                       vnStream stream);
/* steps 1+2 without atomics: every workgroup writes one slab row float[2][C] (vn_bn_bwd_slab_rows(M,C)
 * rows), reduced in double by the finalize — deterministic and ~2x faster than thousands of
 * workgroups adding into the same 2C addresses */
int64_t vn_bn_bwd_slab_rows(int64_t M, int32_t C);
int vn_bn_bwd_reduce_slab(const void *da, vnDtype da_dtype, int64_t da_stride, const void *y,
                          vnDtype y_dtype, int64_t y_stride, int64_t M, int32_t C, const float *stats,
                          int32_t relu, float *slab, vnStream stream);
int vn_bn_bwd_finalize_slab(const float *slab, int64_t slab_rows, int64_t M, int32_t C,
                            const float *gamma, const float *stats, float *coef, float *d_gamma,
                            float *d_beta, vnStream stream);
/* step 3: dy = c0*dz + c1*(y-mean) + c2 -> f32 or bf16 (+ residual at lo_off, as vn_bn_apply) */
int vn_bn_bwd_apply(const void *da, vnDtype da_dtype, int64_t da_stride, const void *y,
                    vnDtype y_dtype, int64_t y_stride, int64_t M, int32_t C, const float *stats,
                    const float *coef, int32_t relu, void *dy, vnDtype dy_dtype, int64_t dy_stride,
                    int64_t lo_off, vnStream stream);
/* BEV-fold variants for the last Conv3d (model.py:262): y / dy are its plain (B*2*H*W, C=64) rows, a / da the
 * (B,1,H,W,2C) tensor block1 sees (row stride wide_stride, channel = d*C + c).  hw = H*W.  One launch each. */
int vn_bn_apply_bev(const void *y, vnDtype y_dtype, int64_t M, int32_t C, int64_t hw, const float *stats,
                    int32_t relu, void *a, vnDtype a_dtype, int64_t wide_stride, vnStream stream);
int vn_bn_bwd_reduce_slab_bev(const void *da, vnDtype da_dtype, int64_t wide_stride, const void *y,
                              vnDtype y_dtype, int64_t M, int32_t C, int64_t hw, const float *stats,
                              int32_t relu, float *slab, vnStream stream);
int vn_bn_bwd_apply_bev(const void *da, vnDtype da_dtype, int64_t wide_stride, const void *y,
                        vnDtype y_dtype, int64_t M, int32_t C, int64_t hw, const float *stats,
                        const float *coef, int32_t relu, void *dy, vnDtype dy_dtype, vnStream stream);
/* Sparse-aware BatchNorm passes of the FIRST middle layer (model.py:207 on the ~99 % empty grid): every output site
 * without an occupied voxel in its receptive field holds exactly the conv bias (`inactive`, float[C]); row_flags are the
 * uint8 site flags vn_active_sites leaves at the head of its workspace.  vn_bn_apply_flagged / _reduce_slab_flagged do
 * not read y at rows with flag 0 (same results as the dense calls); vn_bn_bwd_apply_list writes dy only at the sites of
 * vn_active_sites' list ((b,d,h,w) int64 rows, *count valid, dense contiguous (B,D,H,W,C) tensors). */
int vn_bn_apply_flagged(const void *y, vnDtype y_dtype, int64_t y_stride, int64_t M, int32_t C, const float *stats,
                        int32_t relu, void *a, vnDtype a_dtype, int64_t a_stride, const uint8_t *row_flags,
                        const float *inactive, vnStream stream);
int vn_bn_bwd_reduce_slab_flagged(const void *da, vnDtype da_dtype, int64_t da_stride, const void *y,
                                  vnDtype y_dtype, int64_t y_stride, int64_t M, int32_t C, const float *stats,
                                  int32_t relu, float *slab, const uint8_t *row_flags, const float *inactive,
                                  vnStream stream);
int vn_bn_bwd_apply_list(const void *da, vnDtype da_dtype, const void *y, vnDtype y_dtype, int32_t C, int32_t D,
                         int32_t H, int32_t W, const float *stats, const float *coef, int32_t relu, void *dy,
                         vnDtype dy_dtype, const int64_t *list, const int32_t *count, int64_t cap, vnStream stream);

/* BatchNorm backward of a layer whose output y is the constant inactive[c] outside a site list (the first middle layer,
 * model.py:207 + 142 over the sparse grid of model.py:102-106) WITHOUT the dense gradient of its activation: da_rows is
 * the next layer's data gradient at the listed sites only ([cap][C], list order: vn_conv_gather_gemm_rows with
 * out_linear) and total[c] its sum over ALL sites (vn_dgrad_total).  reduce_list: slab [vn_bn_bwd_list_slab_rows][3][C];
 * finalize_list: coef / d_gamma / d_beta as vn_bn_bwd_finalize_slab; apply_list_rows: dy at the listed sites (dense
 * addressing) as vn_bn_bwd_apply_list.  Same sums as the dense passes (tests/test_gpu_layers.py). */
int64_t vn_bn_bwd_list_slab_rows(int64_t cap, int32_t C);
int vn_bn_bwd_reduce_list(const void *da_rows, vnDtype da_dtype, const void *y, vnDtype y_dtype, int32_t C, int32_t D,
                          int32_t H, int32_t W, const float *stats, int32_t relu, float *slab, const int64_t *list,
                          const int32_t *count, int64_t cap, vnStream stream);
int vn_bn_bwd_finalize_list(const float *slab, int64_t slab_rows, int64_t M, int32_t C, const float *gamma,
                            const float *stats, const float *total, const float *inactive, vnDtype y_dtype,
                            int32_t relu, float *coef, float *d_gamma, float *d_beta, vnStream stream);
int vn_bn_bwd_apply_list_rows(const void *da_rows, vnDtype da_dtype, const void *y, vnDtype y_dtype, int32_t C, int32_t D,
                              int32_t H, int32_t W, const float *stats, const float *coef, int32_t relu, void *dy,
                              vnDtype dy_dtype, const int64_t *list, const int32_t *count, int64_t cap, vnStream stream);
/* total[ci] = the sum over ALL input sites of the data gradient of a 3x3x(kD) convolution (stride 1 and padding 1 in
 * H/W, stride 1 and no padding in D; weight w = the torch (Co,Ci,kD,3,3) fp32 tensor, rounded to bf16 when dy is bf16
 * as the data-gradient kernels read it) — from nine box sums of its dense output gradient dy (B,D,H,W,Co) instead of
 * the dense data gradient (ConvMD backward, model.py:111-167).  dy_sums_to_zero != 0: dy comes out of a train-mode
 * BatchNorm backward (model.py:142), whose per-channel sum over all sites is zero in exact arithmetic: it is taken as
 * zero and only the edge rows / columns of dy are read. */
size_t vn_dgrad_total_workspace_bytes(int32_t Co);
int vn_dgrad_total(const void *dy, vnDtype dy_dtype, int32_t B, int32_t D, int32_t H, int32_t W, int32_t Co, int32_t Ci,
                   int32_t kD, const float *w, int32_t dy_sums_to_zero, void *workspace, size_t workspace_bytes,
                   float *total, vnStream stream);
/* The sparse route for the WEIGHT gradient of the layer above the first middle layer (ConvMD backward, model.py:111-167,
 * for middle_layer.1): its input a = relu(BN(y)) is the constant cvec outside the first layer's site list, so
 *   dW = [weight gradient against the rows a(site) - cvec of the listed sites: vn_act_delta_rows +
 *         vn_conv_wgrad_partials_counted]  +  cvec (x) box sums of dy  [vn_wgrad_const_add, after the unpack].
 * vn_box_col_sums: the box-sum half of vn_dgrad_total alone (same workspace layout). */
int vn_box_col_sums(const void *dy, vnDtype dy_dtype, int32_t B, int32_t D, int32_t H, int32_t W, int32_t Co,
                    void *workspace, size_t workspace_bytes, vnStream stream);
int vn_act_delta_rows(const void *a, vnDtype a_dtype, int32_t C, int32_t D, int32_t H, int32_t W, const float *stats,
                      const float *inactive, vnDtype y_dtype, int32_t relu, const int64_t *list, const int32_t *count,
                      int64_t cap, void *delta_rows, vnDtype delta_dtype, vnStream stream);
int vn_wgrad_const_add(float *dw, const void *workspace, size_t workspace_bytes, int32_t Co, int32_t Ci, int32_t kD,
                       const float *stats, const float *inactive, vnDtype y_dtype, vnDtype a_dtype, int32_t relu,
                       vnStream stream);
/* Row-flag variant for the first middle layer: row_flags = the uint8 site flags vn_active_sites leaves at the head
 * of its workspace ((B,Dr,Hr,Wr) order, 1 = some occupied voxel in the receptive field).  Rows with flag 0 are
 * skipped: that layer's weight- and data-gradient (the row-list kernels) only gather dy at flagged sites. */
int vn_bn_bwd_apply_flagged(const void *da, vnDtype da_dtype, int64_t da_stride, const void *y,
                            vnDtype y_dtype, int64_t y_stride, int64_t M, int32_t C, const float *stats,
                            const float *coef, int32_t relu, void *dy, vnDtype dy_dtype, int64_t dy_stride,
                            const uint8_t *row_flags, vnStream stream);


/* ------------------------------------------------------------------------
 * Layout / dtype helpers at the nn.Module boundary (the reference's modules
 * speak NC(D)HW fp32; model.py:259,262,281).
 * ---------------------------------------------------------------------- */
/* (B,C,S) fp32 -> (B,S,C) rows (f32 / bf16 [+ residual at lo_off]); S = prod(spatial) */
int vn_nchw_to_rows(const float *src, int32_t B, int32_t C, int64_t S, void *dst,
                    vnDtype dst_dtype, int64_t dst_stride, int64_t lo_off, vnStream stream);
/* (B,S,C) rows -> (B,C,S) fp32; sigmoid applied to the first `sigmoid_first_n` channels */
int vn_rows_to_nchw(const void *src, vnDtype src_dtype, int64_t src_stride, int32_t B, int32_t C,
                    int64_t S, float *dst, int32_t sigmoid_first_n, vnStream stream);
/* row-wise cast/copy of M rows of C channels between strided buffers (+ residual at lo_off) */
int vn_cast_rows(const void *src, vnDtype src_dtype, int64_t src_stride, int64_t M, int32_t C,
                 void *dst, vnDtype dst_dtype, int64_t dst_stride, int64_t lo_off, vnStream stream);
/* per-channel column sums of M rows (bias gradients): out[C] = sum_m rows[m,:] (float), two passes through per-
 * workgroup partial rows in the workspace — no atomics: bit-reproducible */
size_t vn_col_sums_workspace_bytes(int64_t M, int32_t C);
int vn_col_sums(const void *rows, vnDtype dtype, int64_t stride, int64_t M, int32_t C,
                float *out, void *workspace, size_t workspace_bytes, vnStream stream);
/* heads epilogue (model.py:281): rows (M,16) = [2 prob logits | 14 reg] ->
 * NCHW prob = sigmoid (B,2,S), reg (B,14,S); and its backward:
 * d_rows = [d_prob * p * (1-p) | d_reg] as f32, bf16 or split bf16 rows */
/* forward side in one launch: rows16 (B*S,16) fp32 (stride 16) -> prob = sigmoid(rows[:, :2]) (B,2,S), reg (B,14,S) */
int vn_heads_to_nchw(const float *rows16, int32_t B, int64_t S, float *prob, float *reg, vnStream stream);
/* The two heads (model.py:276-281) as streaming kernels over the (B*S, 768) bf16 concat rows: forward = product with the
 * packed [16][768] weight (vn_pack_weight mode 0) + bias + sigmoid on channels 0-1, written straight to prob (B,2,S) /
 * reg (B,14,S); data gradient = d_rows (M,16) bf16 times the packed [768][16] weight (mode 1) -> d_cat (M,768) bf16.
 * bf16 only (the fp32 mode keeps vn_conv_gather_gemm + vn_heads_to_nchw). */
int vn_heads_fwd(const void *cat_rows, int64_t cat_stride, const void *w_packed, const float *bias, int32_t B, int64_t S,
                 float *prob, float *reg, vnStream stream);
int vn_heads_dgrad(const void *d_rows, int64_t d_rows_stride, const void *w_packed_dgrad, void *d_cat, int64_t d_cat_stride,
                   int64_t M, vnStream stream);
/* d_cat (M, 768) rows (fp32 or bf16) = d_rows (M,16) fp32 . w (16,768) fp32 (the torch layout of the two heads' weights,
 * score rows first), all products and sums in fp32: no operand rounding in front of the three deconvs' BatchNorm backward */
int vn_heads_dgrad_f32(const float *d_rows, int64_t d_rows_stride, const float *w /*[16][768]*/, void *d_cat,
                       vnDtype d_cat_dtype, int64_t d_cat_stride, int64_t M, vnStream stream);
int vn_heads_bwd(const float *d_prob /*(B,2,S)*/, const float *d_reg /*(B,14,S)*/,
                 const float *prob /*(B,2,S)*/, int32_t B, int64_t S, void *d_rows, vnDtype d_dtype,
                 int64_t d_stride, int32_t split, vnStream stream);

/* ---- RPN loss (voxelnet/model.py:309-352, voxelnet/loss.py:3-13) -----------------------------------------
 * One pass over the (B,h,w) anchor sites for the forward sums and one for the gradients.
 *   prob (B,2,h,w), delta (B,14,h,w): the module's fp32 NCHW outputs (prob after the sigmoid, model.py:281)
 *   pos, neg (B,h,w,2), targets (B,h,w,14): utils.generate_targets' arrays as fp32 channels-last (model.py:309)
 *   out5 = [loss, cls_loss, reg_loss, cls_pos_loss_rec, cls_neg_loss_rec]  (model.py:342-351)
 * vn_rpn_loss_fwd leaves the per-sample normalisers max(1, sum pos), max(1, sum neg) (model.py:313-322) at the
 * head of the workspace; vn_rpn_loss_bwd reads them and the upstream gradients of the five outputs — five device
 * scalars, NULL = 0 (what autograd hands a five-output function; typically only g_loss is set) — and writes
 * d loss / d prob and d loss / d delta. */
size_t vn_rpn_loss_workspace_bytes(int32_t B, int32_t H, int32_t W);
int vn_rpn_loss_fwd(const float *prob, const float *delta, const float *pos, const float *neg,
                    const float *targets, int32_t B, int32_t H, int32_t W, float alpha, float beta, float sigma,
                    void *workspace, size_t workspace_bytes, float *out5, vnStream stream);
int vn_rpn_loss_bwd(const float *prob, const float *delta, const float *pos, const float *neg,
                    const float *targets, int32_t B, int32_t H, int32_t W, float alpha, float beta, float sigma,
                    const void *workspace, const float *g_loss, const float *g_cls, const float *g_reg,
                    const float *g_cls_pos, const float *g_cls_neg, float *d_prob, float *d_delta,
                    vnStream stream);

/* The same loss in three pieces for a caller that schedules them itself (vn_net_step does): the normalisers depend on
 * the target maps only (vn_rpn_loss_norm: any stream, any time before the pass); vn_rpn_loss_fwd_bwd is ONE pass over the
 * sites that leaves the forward partial sums in the workspace AND writes both gradients; vn_rpn_loss_finalize turns the
 * partial sums into out5 (nobody's input in a train step: it need not sit between the network's forward and backward).
 * Same workspace throughout; results bit-identical to vn_rpn_loss_fwd + vn_rpn_loss_bwd. */
int vn_rpn_loss_norm(const float *pos, const float *neg, int32_t B, int32_t H, int32_t W, void *workspace,
                     size_t workspace_bytes, vnStream stream);
int vn_rpn_loss_fwd_bwd(const float *prob, const float *delta, const float *pos, const float *neg,
                        const float *targets, int32_t B, int32_t H, int32_t W, float alpha, float beta, float sigma,
                        void *workspace, size_t workspace_bytes, const float *g_loss, const float *g_cls,
                        const float *g_reg, const float *g_cls_pos, const float *g_cls_neg, float *d_prob,
                        float *d_delta, vnStream stream);
int vn_rpn_loss_finalize(const void *workspace, size_t workspace_bytes, int32_t B, int32_t H, int32_t W, float alpha,
                         float beta, float *out5, vnStream stream);
/* vn_rpn_loss_fwd_bwd with the loss's own upstream gradient only, which ALSO writes the (B*H*W, 16) gradient rows the heads'
 * backward reads — d_logit = d_prob * p * (1 - p) for the two probability columns, then the 14 regression gradients: what
 * vn_heads_bwd makes of d_prob / d_delta / prob, bit for bit (a thread of the pass holds exactly one such row).  vn_net_step
 * uses it: the heads_bwd launch leaves the chain between the loss and the heads' data gradient (model.py:303-304 backward). */
int vn_rpn_loss_fwd_bwd_rows(const float *prob, const float *delta, const float *pos, const float *neg,
                             const float *targets, int32_t B, int32_t H, int32_t W, float alpha, float beta, float sigma,
                             void *workspace, size_t workspace_bytes, const float *g_loss, float *d_prob, float *d_delta,
                             void *d_rows, vnDtype d_dtype, int64_t d_stride, int32_t split, vnStream stream);

/* The objective of the pass as a parameter.  A zeroed spec, or NULL, is the reference's objective above and
 * the vn_rpn_loss_spec_* calls are then the calls they are named after, bit for bit.  Per anchor of a site in sample b, with
 * P_b = max(1, sum pos[b]), eps = 1e-6, fa = focal_alpha, g = focal_gamma:
 *   cls_kind = VN_LOSS_FOCAL (sigmoid focal loss; BOTH terms over the positives' count, the negatives' count is not used):
 *     cls_pos = fa     * pos * (1-p)^g * (-log(p + eps))     / P_b
 *     cls_neg = (1-fa) * neg *   p^g   * (-log(1 - p + eps)) / P_b
 *   yaw_sin = 1 (with either classification objective): the yaw channel's difference goes through the sine,
 *     diff_6 = pos * sin(delta_6 - tgt_6)      instead of      diff_6 = pos * (delta_6 - tgt_6)
 *     (a box and the same box turned by pi cost the same; the heading's sign is then not supervised)
 *   reg_j = smooth_L1(diff_j) / P_b,  j = 0..6, the reference's smooth_L1 (loss.py:3-13) unchanged
 *   out5  = [alpha*S_pos + beta*S_neg + S_reg, alpha*S_pos + beta*S_neg, S_reg, S_pos, S_neg]
 * d_prob is the exact derivative of these expressions (the eps where they stand), d_delta_6 carries cos(delta_6 - tgt_6),
 * the head row is d_prob * p * (1 - p) as before.  p = 0 and p = 1 give finite sums and gradients.
 * focal_gamma must be 0 or >= 1 (0, 1 and 2 are computed by multiplication, other exponents by powf) and focal_alpha in
 * [0,1]: VN_EINVAL otherwise, before anything is launched (the two fields are not read when cls_kind = VN_LOSS_BCE).
 * vn_rpn_loss_spec_check is that test on its own (host only).  vn_rpn_loss_norm, vn_rpn_loss_finalize and
 * vn_rpn_loss_workspace_bytes serve every objective. */
/* (vnLossSpec itself is defined in front of vnStep, whose last member it is) */
int vn_rpn_loss_spec_check(const vnLossSpec *spec);
int vn_rpn_loss_spec_fwd(const float *prob, const float *delta, const float *pos, const float *neg,
                         const float *targets, int32_t B, int32_t H, int32_t W, float alpha, float beta, float sigma,
                         void *workspace, size_t workspace_bytes, float *out5, vnStream stream, const vnLossSpec *spec);
int vn_rpn_loss_spec_bwd(const float *prob, const float *delta, const float *pos, const float *neg,
                         const float *targets, int32_t B, int32_t H, int32_t W, float alpha, float beta, float sigma,
                         const void *workspace, const float *g_loss, const float *g_cls, const float *g_reg,
                         const float *g_cls_pos, const float *g_cls_neg, float *d_prob, float *d_delta,
                         vnStream stream, const vnLossSpec *spec);
int vn_rpn_loss_spec_fwd_bwd(const float *prob, const float *delta, const float *pos, const float *neg,
                             const float *targets, int32_t B, int32_t H, int32_t W, float alpha, float beta, float sigma,
                             void *workspace, size_t workspace_bytes, const float *g_loss, const float *g_cls,
                             const float *g_reg, const float *g_cls_pos, const float *g_cls_neg, float *d_prob,
                             float *d_delta, vnStream stream, const vnLossSpec *spec);
int vn_rpn_loss_spec_fwd_bwd_rows(const float *prob, const float *delta, const float *pos, const float *neg,
                                  const float *targets, int32_t B, int32_t H, int32_t W, float alpha, float beta, float sigma,
                                  void *workspace, size_t workspace_bytes, const float *g_loss, float *d_prob, float *d_delta,
                                  void *d_rows, vnDtype d_dtype, int64_t d_stride, int32_t split, vnStream stream,
                                  const vnLossSpec *spec);

/* ---- rotated-IoU regression loss (csrc/iou_loss.hip) ---------------------------------------------
 * A second regression term beside the smooth-L1 one, on the boxes the regression channels DECODE to.  For every anchor
 * (b, y, x, a), a in {0, 1}, j = (y*W + x)*2 + a, A = anchors[j] = (x, y, z, h, w, l, r) float64 (device; the table
 * vn_rpn_targets and vn_rpn_predict take):
 *   decode(d, A): diag = sqrt(A.w^2 + A.l^2)
 *                 (d0*diag + A.x, d1*diag + A.y, d2*A.h + A.z, exp(d3)*A.h, exp(d4)*A.w, exp(d5)*A.l, d6 + A.r)
 *   P = decode(delta[b, a*7 : a*7+7, y, x], A)      delta   (B,14,H,W) fp32, the module's output
 *   G = decode(targets[b, y, x, a*7 : a*7+7], A)    targets (B,H,W,14) fp32;  m = pos[b, y, x, a], pos (B,H,W,2) fp32
 *   IoU = the iou_bev (metric VN_IOU_BEV) or iou_3d (VN_IOU_3D) of "detection scoring" below: vn_box_iou_rotated(P, G)
 *   kind VN_IOU_LOSS_IOU:   L = 1 - IoU
 *   kind VN_IOU_LOSS_DIOU:  L = 1 - IoU + rho2 / c2
 *        bev: rho2 = (Gx-Px)^2 + (Gy-Py)^2;  c2 = ex^2 + ey^2, ex / ey the extents of the axis-aligned rectangle (lidar
 *             axes) around the 8 footprint corners of P and G
 *        3d:  rho2 += ((Gz + Gh/2) - (Pz + Ph/2))^2;  c2 += ez^2, ez = max(Pz+Ph, Gz+Gh) - min(Pz, Gz)
 *   out2[0] = loss = sum_b (1/P_b) * sum over sample b of m * L,  P_b = max(1, sum pos[b])
 *   out2[1] = mean_iou = (sum m * IoU) / max(1, sum m) over the whole batch (a diagnostic)
 *   d_delta (B,14,H,W) fp32, or NULL for the forward alone = d loss / d delta, times *g when g (a device scalar) is not
 *   NULL.  The derivative runs through the decode (dPx/dd0 = diag, dPh/dd3 = Ph, ...); G is a constant.  EVERY element is
 *   written — zeros where m == 0 — so the buffer need not be cleared.
 * Every float32 input is widened exactly to float64 and all arithmetic is float64 without contraction; only d_delta and
 * out2 are rounded to fp32.  Edge rules:
 *   - a pair scores IoU 0, L = 1 and gradient 0 in BOTH kinds (the distance term is skipped as well) when a decoded
 *     field of P or G is not finite, a size (h, w, l) is not > 0, or a denominator — the sum of the two areas (bev) or
 *     volumes (3d), which bounds area + area - I from above — is <= 0 or not finite;
 *   - the distance term alone is skipped (0, gradient 0) when rho2 or c2 is not finite or c2 <= 0;
 *   - nothing is ever NaN for a finite g and finite pos;
 *   - disjoint boxes (IoU == 0; in 3d also overlapping footprints without z overlap) of kind IOU have gradient exactly 0;
 *   - IoU is piecewise smooth; where it is not (coincident edges, P == G, touching boxes, a tie between two corners for
 *     a side of the enclosing rectangle) d_delta is one of the one-sided derivatives, and finite;
 *   - no work is done where m == 0; the sums take m as a weight, as the smooth-L1 term takes pos.
 * Three launches (normaliser partial sums, the pass over the sites, a one-workgroup finish), sums added in one fixed
 * order: bit-identical from run to run and between the forward-only and the full call.  Asynchronous.
 * VN_EINVAL (before anything is launched or any pointer is read): B, H or W <= 0 or B*H*W >= 2^31, an unknown kind or
 * metric, a NULL delta / pos / targets / anchors / workspace / out2; VN_EWORKSPACE: workspace_bytes below
 * vn_rpn_iou_loss_workspace_bytes(B, H, W) (0 for sizes the call refuses).  Not part of vn_net_step. */
#define VN_IOU_LOSS_IOU 0
#define VN_IOU_LOSS_DIOU 1      /* kind */
#define VN_IOU_BEV 0
#define VN_IOU_3D 1             /* metric: the values vn_box_iou_rotated uses */
size_t vn_rpn_iou_loss_workspace_bytes(int32_t B, int32_t H, int32_t W);
int vn_rpn_iou_loss(const float *delta, const float *pos, const float *targets, const double *anchors /*[H*W*2,7]*/,
                    int32_t B, int32_t H, int32_t W, int32_t kind, int32_t metric, const float *g /*device scalar, NULL = 1*/,
                    void *workspace, size_t workspace_bytes, float *out2, float *d_delta /*NULL: forward only*/, vnStream stream);

/* ---- direction-classifier head (csrc/dir_head.hip) ----------------------------------------------
 * A Conv2d(768, 2, 1) on the concatenation the two heads read: one logit per anchor n = 2*s + a (site s, rotation a)
 * in the site layout of prob, dir[b][a][s]; z > 0 means heading bin 1, z == 0 bin 0.  With pi = the double nearest pi:
 *   wrap_pi(x) = x - floor(x / pi) * pi;   bin(theta) = int(floor((theta - dir_offset) / pi)) & 1   (float64)
 * Rows (cat_rows, d_cat) are VN_BF16 or VN_F32 with a stride in elements >= 768; the base must be 16-byte aligned and the
 * stride a multiple of 16 bytes; w and d_w are [2][768] fp32, w 16-byte aligned.  A split ([hi|lo], VN_F32X3S) or any
 * other row dtype is VN_EINVAL.  B * S rows, B > 0, S > 0, B * S < 2^31.  All four entry points are asynchronous on
 * `stream`, without host synchronisation; none is part of vn_net_step.
 *
 * vn_dir_head_fwd: logits[b][c][s] = bias[c] + sum_k cat_rows[b*S + s][k] * w[c][k] (bias NULL: 0).  fp32 FMAs, 24 per
 * lane in channel order, then a butterfly over 32 lanes: |error| <= 768 * 2^-24 * sum_k |x_k w_k| (+ the bias' rounding).
 *
 * vn_dir_head_bwd: a row whose two d_logits entries are both zero (+0 or -0) is SKIPPED — nothing of it is read or
 * written, its d_cat row included.  The other rows m are listed in row order; with g_c = d_logits[b][c][s]:
 *   d_cat[m][k] = round(d_cat[m][k] + g_0 w[0][k] + g_1 w[1][k])     accumulates; float64 arithmetic, ONE rounding to
 *                                                                    the stored type
 *   d_w[c][k]   = sum_m g_c * cat_rows[m][k];   d_bias[c] = sum_m g_c          (written, not accumulated; 0 without rows)
 * The sums are float64 partials per workgroup over the list in list order, added in index order by a last pass and
 * rounded to fp32 once: no atomics, bit-identical from run to run.  Five launches (count, scan, list, rows, final).
 * VN_EWORKSPACE: workspace_bytes below vn_dir_head_bwd_workspace_bytes(B, S) (0 for sizes the call refuses).
 *
 * vn_rpn_dir_loss (argument order of vn_rpn_iou_loss): logits (B,2,H*W), pos (B,H,W,2), targets (B,H,W,14) fp32, anchors
 * (H*W*2, 7) float64.  theta = (double)targets[b,s,7a+6] + anchors[2s+a][6], t = bin(theta), z = logits[b][a][s]:
 *   out2[0] = L_dir = sum_b (1/P_b) sum m * (max(z,0) - z t + log1p(exp(-|z|))),  m = pos[b,s,a],  P_b = max(1, sum pos[b])
 *   out2[1] = acc   = (sum m * [(z > 0) == t]) / max(1, sum m)                     (a diagnostic)
 *   d_logits (B,2,H*W) or NULL: m * (sigmoid(z) - t) / P_b, and exactly +0.0f where m == 0 (what vn_dir_head_bwd skips);
 *   every element is written.  float64 arithmetic; slab sums added in one fixed order; the scalars are the same bit for
 *   bit with and without d_logits.  VN_EINVAL also for a dir_offset that is not finite; VN_EWORKSPACE as above.
 *
 * vn_boxes_rectify_yaw: boxes (B,K,7) in place, idx (B,K) the anchor index n as vn_rpn_select_decode_layout writes it
 * with VN_DETECT_SITE, counts (B), dir_logits (B,2,n_anchors/2).  For the first min(counts[b], K) rows of sample b:
 *   boxes[b][k][6] = wrap_pi(r - dir_offset) + dir_offset + pi * [dir_logits[b][n & 1][n >> 1] > 0]      (float64)
 * Nothing else is written; a row whose idx is not in [0, n_anchors) is left as it is.  Both operations turn the box by
 * a multiple of pi: the footprint, every IoU and a suppression's outcome stay.  VN_EINVAL: B, K or n_anchors <= 0, an
 * odd n_anchors, a dir_offset that is not finite, a NULL pointer. */
int vn_dir_head_fwd(const void *cat_rows, int32_t dtype, int64_t cat_stride, const float *w /*[2][768]*/,
                    const float *bias /*[2] or NULL*/, int32_t B, int64_t S, float *logits /*[B][2][S]*/, vnStream stream);
size_t vn_dir_head_bwd_workspace_bytes(int32_t B, int64_t S);
int vn_dir_head_bwd(const float *d_logits /*[B][2][S]*/, const void *cat_rows, int32_t dtype, int64_t cat_stride,
                    const float *w /*[2][768]*/, int32_t B, int64_t S, void *d_cat, int32_t d_cat_dtype, int64_t d_cat_stride,
                    float *d_w /*[2][768]*/, float *d_bias /*[2]*/, void *workspace, size_t workspace_bytes, vnStream stream);
size_t vn_rpn_dir_loss_workspace_bytes(int32_t B, int32_t H, int32_t W);
int vn_rpn_dir_loss(const float *logits, const float *pos, const float *targets, const double *anchors /*[H*W*2,7]*/,
                    int32_t B, int32_t H, int32_t W, double dir_offset, void *workspace, size_t workspace_bytes,
                    float *out2, float *d_logits /*NULL: forward only*/, vnStream stream);
int vn_boxes_rectify_yaw(float *boxes /*[B][K][7]*/, const int32_t *idx /*[B][K]*/, const int32_t *counts /*[B]*/,
                         const float *dir_logits /*[B][2][n_anchors/2]*/, int32_t B, int32_t K, int32_t n_anchors,
                         double dir_offset, vnStream stream);

/* ---- IoU-aware confidence head (csrc/iou_head.hip) -----------------------------------------------
 * A second Conv2d(768, 2, 1) on the concatenation: z[b][a][s], the site layout of prob and of the direction logits,
 * q = sigmoid(z) predicts the IoU of anchor n = 2*s + a's decoded box with its ground truth.  The head's forward and
 * backward are vn_dir_head_fwd / vn_dir_head_bwd.  All three entry points are asynchronous on `stream`, without host
 * synchronisation; none is part of vn_net_step.
 *
 * vn_rpn_iou_head_loss: logits (B,2,H*W), delta (B,14,H,W), pos (B,H,W,2), targets (B,H,W,14) fp32, anchors (H*W*2, 7)
 * float64.  With P = decode(delta[b, 7a..7a+6, s], A_n), G = decode(targets[b, s, 7a..7a+6], A_n) (vn_rpn_iou_loss'
 * decode and validity rules: an invalid pair scores 0) and t = clamp(IoU_metric(P, G), 0, 1), a CONSTANT:
 *   out2[0] = L   = sum_b (1/P_b) sum m * (max(z,0) - z t + log1p(exp(-|z|))),  m = pos[b,s,a],  P_b = max(1, sum pos[b])
 *   out2[1] = mae = (sum m * |q - t|) / max(1, sum m)                            (a diagnostic)
 *   d_logits (B,2,H*W) or NULL: m * (q - t) / P_b, and exactly +0.0f where m == 0 (what vn_dir_head_bwd skips)
 *   iou_target (B,2,H*W) or NULL: (float)t where m != 0, +0.0f elsewhere
 * Every element of the two maps is written; there is NO gradient for delta.  float64 arithmetic, nothing is read where
 * m == 0; slab sums added in one fixed order: bit-identical from run to run and with or without the optional outputs.
 * VN_EINVAL: B, H or W <= 0 or B*H*W >= 2^31, an unknown metric (VN_IOU_BEV / VN_IOU_3D), a NULL logits / delta / pos /
 * targets / anchors / workspace / out2; VN_EWORKSPACE: workspace_bytes below vn_rpn_iou_head_loss_workspace_bytes.
 *
 * vn_iou_rectify_probs: out[i] = (float)(pow((double)probs[i], 1 - alpha) * pow(sigmoid((double)iou_logits[i]), alpha)),
 * i < n = B*2*S, elementwise in the site layout; alpha == 0 copies probs bit for bit.  out must not be probs.
 * VN_EINVAL: n <= 0 or >= 2^31, alpha outside [0, 1] or not finite, a NULL pointer, out == probs.
 *
 * vn_site_heads_fwd: vn_dir_head_fwd for n_out = 2 or 4 outputs in ONE read of the rows: w [n_out][768] (16-byte aligned),
 * bias [n_out] or NULL, logits [B][n_out][S].  Output c has the bits vn_dir_head_fwd gives for weight row c (the same
 * FMAs in the same order, the same butterfly).  Rows as for vn_dir_head_fwd; VN_EINVAL also for any other n_out. */
size_t vn_rpn_iou_head_loss_workspace_bytes(int32_t B, int32_t H, int32_t W);
int vn_rpn_iou_head_loss(const float *logits /*[B][2][H*W]*/, const float *delta, const float *pos, const float *targets,
                         const double *anchors /*[H*W*2,7]*/, int32_t B, int32_t H, int32_t W, int32_t metric, void *workspace,
                         size_t workspace_bytes, float *out2, float *d_logits /*NULL: forward only*/,
                         float *iou_target /*[B][2][H*W] or NULL*/, vnStream stream);
int vn_iou_rectify_probs(const float *probs, const float *iou_logits, int64_t n, double alpha, float *out, vnStream stream);
int vn_site_heads_fwd(const void *cat_rows, int32_t dtype, int64_t cat_stride, const float *w /*[n_out][768]*/,
                      const float *bias /*[n_out] or NULL*/, int32_t n_out, int32_t B, int64_t S,
                      float *logits /*[B][n_out][S]*/, vnStream stream);

/* ---- optimizer tail (voxelnet/train.py:153-154 with the optimizer of train.py:130-132) ---------------------
 * torch.nn.utils.clip_grad_norm_(parameters, max_norm) followed by an update rule, in two launches.  The clip is the
 * same code under both rules (vn_clip_sgd here, vn_clip_adamw below):
 *   total = sqrt(sum |g|^2) over EVERY chunk;  coef = min(1, max_norm / (total + 1e-6))  (NaN stays NaN);  g' = g * coef
 * Sums: fp32 per thread, one fp32 partial per chunk, added in double in one fixed order by every workgroup of the second
 * launch — no atomics, bit-identical from run to run.  scale_grads != 0 also stores g' (what clip_grad_norm_ leaves
 * behind); total_norm (device, may be NULL) receives the norm before clipping, clip_grad_norm_'s return value.
 * vn_clip_sgd: SGD(lr) without momentum / weight decay, p -= lr * g'.  `chunks` is a DEVICE array the caller builds once
 * for a fixed set of fp32 tensors: every (parameter, gradient) pair cut into pieces of at most VN_OPT_CHUNK elements. */
#define VN_OPT_CHUNK 4096
typedef struct vnParamChunk {
    float *param;
    float *grad;
    int32_t n;          /* elements in this piece, 1..VN_OPT_CHUNK */
    int32_t reserved;
} vnParamChunk;
size_t vn_clip_sgd_workspace_bytes(int32_t n_chunks);
int vn_clip_sgd(const vnParamChunk *chunks, int32_t n_chunks, float max_norm, float lr, int32_t scale_grads,
                void *workspace, size_t workspace_bytes, float *total_norm, vnStream stream);

/* ---- optimizer tail with AdamW in SGD's place (voxelnet/train.py:153-154; what every successor trains with) ----
 * The clip of vn_clip_sgd (above: norm over every chunk whatever its slot, coefficient, sums, scale_grads, total_norm)
 * followed by torch.optim.AdamW's update (torch/optim/adam.py _single_tensor_adam with decoupled_weight_decay, amsgrad =
 * False, maximize = False), in two launches; per element, with the values of its chunk's slot:
 *     p *= 1 - lr * wd;  m += (g' - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * g'^2
 *     p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * `chunks` is a DEVICE array built once for a fixed set of fp32 tensors: every (parameter, gradient, exp_avg, exp_avg_sq)
 * quadruple cut into pieces of at most VN_OPT_CHUNK elements, each naming the hyperparameter slot it takes; the kernel
 * clamps that index into [0, n_slots).  `hyper` is HOST memory, read during the call and not afterwards: lr, the betas
 * and the step count can change from call to call (schedulers) without touching the device table.  The slot's five
 * floats are widened to the double with the shortest decimal form that rounds to the float (0.999f means 0.999, not
 * 0.99900001287...), 1 - beta, 1 - lr * wd and 1 - beta^t are taken in double, and the results go to the kernel by value.
 * VN_EINVAL (before any HIP call): a NULL chunks / hyper / workspace, n_chunks <= 0, max_norm <= 0 or NaN, n_slots outside
 * 1..VN_OPT_MAX_SLOTS, a slot (of the first n_slots) with a beta outside [0,1), eps < 0, lr < 0, weight_decay < 0, step < 1
 * or a NaN; VN_EWORKSPACE: workspace_bytes < vn_clip_adamw_workspace_bytes(n_chunks).  Asynchronous. */
#define VN_OPT_MAX_SLOTS 8
typedef struct vnAdamChunk {
    float *param;
    float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int32_t n;          /* elements in this piece, 1..VN_OPT_CHUNK */
    int32_t slot;       /* index into vnAdamHyper.slot */
} vnAdamChunk;
typedef struct vnAdamSlot {
    float lr, beta1, beta2, eps, weight_decay;
    int32_t step;       /* t >= 1: the step being taken */
} vnAdamSlot;
typedef struct vnAdamHyper {
    int32_t n_slots;
    vnAdamSlot slot[VN_OPT_MAX_SLOTS];
} vnAdamHyper;
size_t vn_clip_adamw_workspace_bytes(int32_t n_chunks);
int vn_clip_adamw(const vnAdamChunk *chunks, int32_t n_chunks, const vnAdamHyper *hyper, float max_norm,
                  int32_t scale_grads, void *workspace, size_t workspace_bytes, float *total_norm, vnStream stream);

/* ---- exponential moving average of the weights (timm ModelEmaV2, torch.optim.swa_utils) --------
 *     ema = lerp(ema, x, weight),  weight = 1 - decay, handed over by value (the schedule is the caller's)
 * with torch.lerp's rounding: d = x - ema;  weight < 0.5: fmaf(weight, d, ema);  otherwise: fmaf(-d, 1 - weight, x) — the
 * form the AdamW rule uses for exp_avg, one piece of code for both.  weight = 1 copies x, weight = 0 keeps ema (finite
 * values).  Three entry points:
 * vn_ema_update: ONE launch over a DEVICE table of (source, shadow) pieces of at most VN_OPT_CHUNK fp32 elements, one
 *   workgroup per piece, no workspace.  For what no update rule touches (BatchNorm running statistics, parameters without
 *   a gradient) and for callers with an optimizer of their own.
 * vn_clip_sgd_ema / vn_clip_adamw_ema: vn_clip_sgd / vn_clip_adamw with one more pointer per chunk; the second launch
 *   averages the parameter value it has just computed (from the register: not read again) into `ema`.  p, the moments,
 *   the stored gradients and total_norm are those of the plain entry points bit for bit, and the shadow is what
 *   vn_ema_update over the same tensors right after the plain call gives, bit for bit.  Workspace: that of
 *   vn_clip_sgd_workspace_bytes / vn_clip_adamw_workspace_bytes.
 * A piece whose `ema` (or, for vn_ema_update, `src`) is NULL is left out of the average.  16-byte accesses where every
 * pointer of the piece allows them, element by element otherwise.
 * VN_EINVAL (before any HIP call): what the plain entry point refuses; a weight outside [0,1] or NaN; for vn_ema_update a
 * NULL chunks or n_chunks <= 0.  Asynchronous. */
typedef struct vnEmaChunk {
    const float *src;
    float *ema;
    int32_t n;          /* elements in this piece, 1..VN_OPT_CHUNK */
    int32_t reserved;
} vnEmaChunk;
typedef struct vnParamChunkEma {
    float *param;
    float *grad;
    float *ema;         /* NULL: no average for this piece */
    int32_t n;          /* elements in this piece, 1..VN_OPT_CHUNK */
    int32_t reserved;
} vnParamChunkEma;
typedef struct vnAdamChunkEma {
    float *param;
    float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    float *ema;         /* NULL: no average for this piece */
    int32_t n;          /* elements in this piece, 1..VN_OPT_CHUNK */
    int32_t slot;       /* index into vnAdamHyper.slot */
} vnAdamChunkEma;
int vn_ema_update(const vnEmaChunk *chunks, int32_t n_chunks, float weight, vnStream stream);
int vn_clip_sgd_ema(const vnParamChunkEma *chunks, int32_t n_chunks, float max_norm, float lr, int32_t scale_grads,
                    float ema_weight, void *workspace, size_t workspace_bytes, float *total_norm, vnStream stream);
int vn_clip_adamw_ema(const vnAdamChunkEma *chunks, int32_t n_chunks, const vnAdamHyper *hyper, float max_norm,
                      int32_t scale_grads, float ema_weight, void *workspace, size_t workspace_bytes, float *total_norm,
                      vnStream stream);

/* ---- RPN training targets (voxelnet/utils.py:376-473 generate_targets, :344-373 bbox_iou, :213-227
 * anchor_to_standup_box2d; called by RPN3D.forward, voxelnet/model.py:309) -------------------------------
 * Per sample b: gt_count[b] ground-truth boxes in lidar coordinates, gt [B,max_gt,7] = (x,y,z,h,w,l,r) float64 and
 * their stand-up rectangles gt_standup [B,max_gt,4] = (x1,y1,x2,y2) float32 (utils.label_to_gt_box_3d and
 * corner_to_standup_box2d(center_to_corner_box_2d(.)) on the host: O(boxes) work).  anchors [n_anchors,7] float64 is
 * utils.generate_anchors().reshape(-1,7): anchor n = (iy*W + ix)*2 + rotation.
 * Outputs in the reference's channels-last layouts: pos, neg [B,n_anchors] == (B,h,w,2); targets [B,n_anchors,7] ==
 * (B,h,w,14); float32 (model.py:327-329 converts the float64 arrays).  Which anchors are positive / negative is
 * bit-exact with the reference, its IoU quirks included; regression targets are float64 arithmetic rounded to fp32. */
#define VN_TARGETS_MAX_GT 128
size_t vn_rpn_targets_workspace_bytes(int32_t B, int32_t n_anchors, int32_t max_gt);
int vn_rpn_targets(const double *anchors, int32_t n_anchors, const double *gt, const float *gt_standup,
                   const int32_t *gt_count /*device [B]*/, int32_t B, int32_t max_gt, float pos_iou, float neg_iou,
                   double anchor_h, float *pos, float *neg, float *targets, void *workspace, size_t workspace_bytes,
                   vnStream stream);

/* ---- RPN training targets by a real IoU (csrc/targets_iou.hip; rules and the reason: DESIGN.md section 1h) ----
 * vn_rpn_targets above keeps the reference's assignment, whose anchor rectangles have zero extent and whose union
 * term depends on where the anchor lies relative to the line y = x.  vn_rpn_targets_iou takes the same anchors, gt,
 * gt_count, thresholds and output maps (no gt_standup: nothing is prepared on the host) and assigns by IoU(n,k) of
 * anchor n and box k, float64 throughout, the two thresholds being the float arguments widened to double:
 *   VN_ASSIGN_STANDUP: the axis-aligned hulls of the two rotated footprints — box (x, y, w, l, r) has the hull
 *                      x +- hx, y +- hy, hx = (l|cos r| + w|sin r|)/2, hy = (l|sin r| + w|cos r|)/2, area 2hx * 2hy (no
 *                      "+1"); iw, ih = the hulls' overlap along x, y, written from the centres: iw = min(hx_n + hx_k -
 *                      |x_k - x_n|, 2 min(hx_n, hx_k)), so that anchors which all contain a box's hull along an axis (or
 *                      lie inside it) tie exactly instead of by rounding; IoU = iw*ih / (area_n + area_k - iw*ih); 0
 *                      when iw <= 0 or ih <= 0 (and for a non-finite result).
 *   VN_ASSIGN_ROTATED: iou_bev of the detection scoring below for the pair (anchor, box): 0, never NaN, for a box with a
 *                      non-finite field or h, w or l <= 0.
 * m_n = max_k IoU(n,k), k_n = the smallest k that attains it;  M_k = max_n IoU(n,k), n_k = the smallest n that attains it.
 *   matched[n] = k_n when m_n >= pos_iou; else the smallest k with n_k == n and M_k > 0 (a box whose best anchor stays
 *                below pos_iou still gets that one anchor); else -1.        [B,n_anchors] int32, or NULL
 *   pos = matched >= 0;  neg = m_n < neg_iou and not pos: the two are exclusive, unlike vn_rpn_targets'.  Every anchor of
 *   a sample without a box is negative.
 *   targets: k_tg_encode's seven expressions on gt[matched[n]], float64 rounded to float32; zeros for a non-positive.
 * Limits as vn_rpn_targets (max_gt <= VN_TARGETS_MAX_GT, B * n_anchors < 2^28); gt_count is clamped to [0, max_gt] on
 * the device.  VN_EINVAL, before anything is launched, for a size outside the limits, a null pointer (matched
 * excepted), an unknown iou_kind, a NaN threshold or anchor_h == 0; VN_EWORKSPACE for a workspace below the query's
 * answer (0 for unsupported sizes).  Asynchronous on `stream`, no host synchronisation; integer atomics of
 * order-independent results only: outputs are bit-identical from run to run. */
#define VN_ASSIGN_STANDUP 1
#define VN_ASSIGN_ROTATED 2
size_t vn_rpn_targets_iou_workspace_bytes(int32_t B, int32_t n_anchors, int32_t max_gt);
int vn_rpn_targets_iou(const double *anchors, int32_t n_anchors, const double *gt /*[B,max_gt,7]*/,
                       const int32_t *gt_count /*device [B]*/, int32_t B, int32_t max_gt, int32_t iou_kind,
                       float pos_iou, float neg_iou, double anchor_h, float *pos, float *neg, float *targets,
                       int32_t *matched /*[B,n_anchors] ground-truth index or -1; may be NULL*/, void *workspace,
                       size_t workspace_bytes, vnStream stream);

/* ---- RPN training targets by ATSS (csrc/targets_atss.hip) -------------------------------------------
 * Adaptive Training Sample Selection (Zhang et al., CVPR 2020): instead of the two fixed thresholds of the calls above,
 * every ground-truth box takes the anchors nearest to it as candidates and sets its own IoU threshold from them.  Same
 * anchors, gt, gt_count and output maps as vn_rpn_targets_iou; the anchors' two rotations stand for the paper's pyramid
 * levels.  All arithmetic is float64.
 * Inputs: anchors [n_anchors,7], anchor n = site * 2 + rotation, n_anchors even; group a = the anchors with (n & 1) == a.
 *   gt [B,max_gt,7] = (x, y, z, h, w, l, r); gt_count[b] (device) is clamped to [0, max_gt]; 1 <= top_k <= VN_ATSS_MAX_TOPK.
 * Validity: box k of sample b is valid when k < gt_count[b], all seven fields are finite and h, w, l > 0.  An invalid box has
 *   no candidates, makes no positive and gets stats of zeros.
 * For a valid box k:
 *   1. d2(n,k) = dx*dx + dy*dy with dx = x_n - x_k, dy = y_n - y_k (a NaN d2 — an anchor without a position — counts as +inf).
 *   2. C_k = the union over the two groups of the min(top_k, n_anchors / 2) anchors of the group with the smallest (d2, n)
 *      in lexicographic order: equal d2 goes to the smaller n.  |C_k| = 2 min(top_k, n_anchors / 2) >= 2.
 *   3. v(n,k) for n in C_k: the IoU of iou_kind (VN_ASSIGN_STANDUP or VN_ASSIGN_ROTATED) exactly as vn_rpn_targets_iou
 *      computes it for the pair — the same device functions.
 *   4. mu_k = sum(v) / |C_k|;  sd_k = sqrt(sum((v - mu_k)^2) / (|C_k| - 1)) (the unbiased estimate, the published code's
 *      std);  t_k = mu_k + sd_k.  Both sums run over C_k in one fixed order: group 0's candidates by ascending (d2, n),
 *      then group 1's.
 *   5. Box k accepts n in C_k when v(n,k) >= t_k, v(n,k) > 0 and the anchor's centre lies inside the box's bird's-eye
 *      footprint: with c = cos r_k, s = sin r_k, u = dx*c + dy*s (along the box's LENGTH l, its local x axis) and
 *      w' = -(dx*s) + dy*c (along its WIDTH w), |u| <= l/2 and |w'| <= w/2 — the edge is inside.  (The footprint of
 *      vn_box_iou_rotated and vn_points_in_boxes: l along the heading r, w across it.)
 *   6. matched[n] = the box that accepted n with the largest v(n,k), the smallest k among equals; -1 when none did.
 *      [B,n_anchors] int32, or NULL.  pos = matched >= 0;  neg = not pos: there is no ignore band and no forced positive,
 *      and every anchor of a sample without a box is negative.
 *      targets: vn_rpn_targets_iou's encoding of gt[matched[n]] on anchor n, float64 rounded to float32; zeros for a
 *      non-positive.
 *   7. stats [B,max_gt,4] float64, or NULL: (mu_k, sd_k, t_k, the number of anchors with matched == k); zeros for an invalid
 *      box and for k >= gt_count[b].  A box that ends with no anchor — off the grid (every v is 0, stats all zero), or no
 *      candidate centre inside it — is plain ATSS behaviour and shows here.
 * Limits as vn_rpn_targets_iou.  VN_EINVAL, before anything is launched, for a size outside the limits, an odd n_anchors,
 * top_k outside its range, an unknown iou_kind, a null pointer (matched and stats excepted) or anchor_h == 0; VN_EWORKSPACE
 * for a workspace below the query's answer (0 for unsupported sizes).  Asynchronous on `stream`, no host synchronisation;
 * no floating-point atomics, integer atomics of order-independent results only: outputs are bit-identical from run to run. */
#define VN_ATSS_MAX_TOPK 32
size_t vn_rpn_targets_atss_workspace_bytes(int32_t B, int32_t n_anchors, int32_t max_gt, int32_t top_k);
int vn_rpn_targets_atss(const double *anchors, int32_t n_anchors, const double *gt /*[B,max_gt,7]*/,
                        const int32_t *gt_count /*device [B]*/, int32_t B, int32_t max_gt, int32_t iou_kind, int32_t top_k,
                        double anchor_h, float *pos, float *neg, float *targets, int32_t *matched /*may be NULL*/,
                        double *stats /*[B,max_gt,4]; may be NULL*/, void *workspace, size_t workspace_bytes,
                        vnStream stream);

/* ---- RPN training targets by SimOTA (csrc/targets_ota.hip) ------------------------------------------
 * The prediction-aware dynamic-k assignment of YOLOX (Ge et al., 2021): a ground-truth box takes the anchors whose CURRENT
 * PREDICTION fits it best, and how many it takes follows from how many predictions already overlap it.  Same anchors, gt,
 * gt_count and output maps as vn_rpn_targets_atss; unlike its three siblings the call reads the network's outputs, so it
 * runs after the forward.  All arithmetic is float64; every float32 input is widened exactly.
 * Inputs: anchors [n_anchors,7], anchor n = 2 * site + a, n_anchors even, S = n_anchors / 2 sites.  gt [B,max_gt,7];
 *   gt_count[b] (device) is clamped to [0, max_gt].  probs [B,2,S] and deltas [B,14,S] float32 in the SITE layout — the
 *   module's NCHW outputs as they lie in memory: anchor (s, a) has p = probs[b,a,s] and d_j = deltas[b,7a+j,s], j = 0..6.
 *   1 <= q <= VN_OTA_MAX_Q (YOLOX: 10); radius >= 0, finite, in metres; iou_weight >= 0, finite (YOLOX: 3); metric
 *   VN_IOU_BEV or VN_IOU_3D.
 * Validity as in vn_rpn_targets_atss: box k of sample b is valid when k < gt_count[b], all seven fields are finite and
 *   h, w, l > 0.  For a valid box k and anchor n, dx = x_n - x_k, dy = y_n - y_k, c = cos r_k, s = sin r_k,
 *   u = dx*c + dy*s, w' = -(dx*s) + dy*c (vn_rpn_targets_atss rules 1 and 5, the same expressions):
 *   1. in_box(n,k): |u| <= l/2 and |w'| <= w/2, edges inside — the footprint test of vn_rpn_targets_atss rule 5.
 *   2. in_ctr(n,k): |dx| <= radius and |dy| <= radius, edges inside; a NaN compares false.
 *   3. Candidates: C_k = {n : in_box(n,k) or in_ctr(n,k)}.  There is no bound on |C_k|.
 *   4. P(n) = the box d decodes to on anchor n (the decode of vn_rpn_iou_loss: x, y by the anchor's diagonal, z by its
 *      height, sizes by exp, yaw added).  v(n,k) = the iou_bev / iou_3d of "detection scoring" below for (P(n), gt_k): 0,
 *      never NaN, when a decoded field is not finite or a size is <= 0.
 *   5. cost(n,k) = -log(pc) + iou_weight * (-log(v + 1e-8)) + (in_box and in_ctr ? 0 : 1e5), the three terms added left to
 *      right; pc = min(max(p, 1e-12), 1), a NaN p counts as 1e-12.
 *   6. m = min(q, |C_k|); sum_k = the sum of the m largest v over C_k, added in descending order (equal values in any
 *      order: the sum is the same); dyn_k = max(1, int(floor(sum_k))), which is <= m because v <= 1.
 *   7. Box k selects the dyn_k candidates with the smallest (cost, n), lexicographic.
 *   8. matched[n] = the selecting box of the smallest cost(n,k), the smallest k among equals; -1 when none selected n.
 *      An anchor lost to another box is not replaced (plain SimOTA), so a box may end with fewer than dyn_k anchors, or none.
 *   9. pos = matched >= 0; neg = not pos.
 *  10. targets: vn_rpn_targets_iou's encoding of gt[matched[n]] on anchor n, float64 rounded to float32; zeros for a
 *      non-positive.
 *  11. stats [B,max_gt,5] float64, or NULL: (|C_k|, sum_k, dyn_k, the cost of the last selected candidate, the number of
 *      anchors with matched == k); zeros for an invalid box, for k >= gt_count[b] and for a box with no candidate.
 * Limits as vn_rpn_targets_atss.  VN_EINVAL, before anything is launched, for a size outside the limits, an odd n_anchors,
 * q outside its range, a NaN, negative or infinite radius or iou_weight, an unknown metric, a null pointer (matched and
 * stats excepted) or anchor_h == 0; VN_EWORKSPACE for a workspace below the query's answer (0 for unsupported sizes).
 * Asynchronous on `stream`, no host synchronisation; no floating-point atomics, integer atomics of order-independent
 * results only: outputs are bit-identical from run to run. */
#define VN_OTA_MAX_Q 16
size_t vn_rpn_targets_ota_workspace_bytes(int32_t B, int32_t n_anchors, int32_t max_gt, int32_t q);
int vn_rpn_targets_ota(const double *anchors, int32_t n_anchors, const double *gt /*[B,max_gt,7]*/,
                       const int32_t *gt_count /*device [B]*/, int32_t B, int32_t max_gt, const float *probs /*[B,2,S]*/,
                       const float *deltas /*[B,14,S]*/, int32_t metric, int32_t q, double radius, double iou_weight,
                       double anchor_h, float *pos, float *neg, float *targets, int32_t *matched /*may be NULL*/,
                       double *stats /*[B,max_gt,5]; may be NULL*/, void *workspace, size_t workspace_bytes,
                       vnStream stream);

/* ---- inference tail (voxelnet/model.py:364-395 RPN3D.predict: utils.deltas_to_boxes_3d utils.py:476-489,
 * filter_boxes model.py:28-57, utils.nms utils.py:492-553) ----------------------------------------------
 * probs (B,2,h,w) and deltas (B,14,h,w): the module's fp32 NCHW outputs, read as the flat (B, n_anchors) and
 * (B, n_anchors, 7) views the reference's reshapes take (no permute: utils.py:478, model.py:384); anchors
 * [n_anchors,7] float64.  Per sample: boxes [top_k,7] (x,y,z,h,w,l,r) and scores [top_k] of the kept detections in
 * descending score, counts[b] of them valid.  score_thres = cfg.RPN.SCORE_THRES (>= keeps), nms_thres =
 * cfg.RPN.NMS_THRES, top_k = cfg.RPN.NMS_POST_TOPK <= VN_PREDICT_MAX_TOPK. */
#define VN_PREDICT_MAX_TOPK 64
size_t vn_rpn_predict_workspace_bytes(int32_t B, int32_t n_anchors);
int vn_rpn_predict(const float *probs, const float *deltas, const double *anchors, int32_t B, int32_t n_anchors,
                   float score_thres, double nms_thres, int32_t top_k, double anchor_h, float *boxes, float *scores,
                   int32_t *counts, void *workspace, size_t workspace_bytes, vnStream stream);

/* ---- detection scoring (eval.py:4-5 is empty in the reference; protocol: DESIGN.md section 1b) --------------
 * Box = (x, y, z, h, w, l, r), lidar frame: footprint corners (+-l/2, +-w/2) turned by r about (x, y), vertical
 * extent [z, z+h].  All IoU arithmetic is float64 (csrc/eval.hip).
 *   BEV intersection I: both footprints translated so that A's centre is the origin, A's rectangle clipped by the
 *   four half-planes of B (Sutherland-Hodgman), shoelace area.
 *   iou_bev = I / (wa*la + wb*lb - I);   iou_3d = I*zo / (ha*wa*la + hb*wb*lb - I*zo),
 *   zo = max(0, min(za+ha, zb+hb) - max(za, zb)).  A pair scores 0, never NaN, when a field is not finite, when w, l
 *   or h of either box is <= 0, or when the denominator is <= 0.
 * vn_box_iou_rotated: a [na,7], b [nb,7] float64 (device) -> out [na,nb] float64; metric VN_EVAL_BEV / VN_EVAL_3D
 * (VN_EINVAL otherwise); na == 0 or nb == 0 is a no-op.  One thread per pair, no workspace, asynchronous.
 *
 * vn_eval_match: per frame b, the greedy matching of vn_rpn_predict's outputs (det_boxes [B,top_k,7] and det_scores
 * [B,top_k] float32, det_counts [B] read ON THE DEVICE) against gt [B,max_gt,7] float64 with gt_counts [B] (device)
 * and gt_flags [B,n_diff,max_gt] (0 valid, anything else ignored), for both metrics and every one of the n_diff
 * difficulties: detections by descending score (ties: lower index); a detection takes, among the ground truths not
 * taken yet with IoU > thr, the valid one with the largest IoU (ties: lowest index), else the ignored one with the
 * largest IoU; a taken ground truth, valid or ignored, is gone for the later detections.
 *   status     [B,2,n_diff,top_k] int8 : 1 TP (took a valid one), 0 FP, -1 ignored (took an ignored one), -2 slot
 *                                        beyond det_counts[b];  axis 1: VN_EVAL_BEV, VN_EVAL_3D
 *   matched_gt [B,2,n_diff,top_k] int32: index of the taken ground truth, -1 none
 *   iou_out    [B,2,top_k,max_gt] float64 or NULL: the frame's IoU tables (0 beyond the counts)
 *   workspace  vn_eval_match_workspace_bytes(B, top_k, max_gt) bytes; afterwards its first B*top_k int32 hold the
 *              order in which each frame's detections were walked (-1 beyond the count)
 * One workgroup per frame, one launch, no host synchronisation.  Limits: 1 <= top_k <= VN_EVAL_MAX_TOPK, 1 <= max_gt
 * <= VN_TARGETS_MAX_GT, 1 <= n_diff <= VN_EVAL_MAX_DIFF.  VN_EINVAL for a size outside them, a NaN threshold, a null
 * pointer (iou_out excepted) or a workspace smaller than asked for; B == 0 is a no-op (0).  Counts outside
 * [0, top_k] / [0, max_gt] are clamped on the device. */
#define VN_EVAL_MAX_TOPK 32
#define VN_EVAL_MAX_DIFF 8
#define VN_EVAL_BEV 0
#define VN_EVAL_3D 1
int vn_box_iou_rotated(const double *a, int32_t na, const double *b, int32_t nb, int32_t metric, double *out,
                       vnStream stream);
size_t vn_eval_match_workspace_bytes(int32_t B, int32_t top_k, int32_t max_gt);
int vn_eval_match(const float *det_boxes, const float *det_scores, const int32_t *det_counts, const double *gt,
                  const int32_t *gt_counts, const uint8_t *gt_flags, int32_t B, int32_t top_k, int32_t max_gt,
                  int32_t n_diff, double thr_bev, double thr_3d, int8_t *status, int32_t *matched_gt, double *iou_out,
                  void *workspace, size_t workspace_bytes, vnStream stream);

/* ---- image-plane scoring (eval.py:4-5 is empty in the reference; rules: DESIGN.md section 1b-bis, which restates
 * the image-plane rules of KITTI's object devkit: 2D AP, AOS, DontCare regions, the 2D-height bar) ----------------
 * vn_boxes_to_image: one thread per detection slot.  det_boxes [B,top_k,7] float32 lidar boxes, det_counts [B] read ON
 * THE DEVICE, calib [B,24] float64 = per frame [M | P2], both 3x4 row-major, M = (R0_rect . Tr_velo_to_cam)[:3],
 * image_hw [B,2] int32 = (H, W).  All arithmetic float64.
 *   centre c = M.(x,y,z,1);  ry = wrap(-r - pi/2);  alpha = wrap(ry - atan2(c_x, c_z));  wrap: into (-pi, pi]
 *   the eight corners of the LIDAR-frame box (footprint (+-l/2, +-w/2) turned by r about (x, y), at z and z + h) map by
 *   q = P2.(M.corner, 1), u = q0/q2, v = q1/q2, depth q2;  x1 = max(min u, 0), y1 = max(min v, 0),
 *   x2 = min(max u, W-1), y2 = min(max v, H-1)
 *   on the image <=> every field finite, h, w, l > 0, all eight depths > 0.1, x2 > x1 and y2 > y1
 *   rows     [B,top_k,VN_EVAL_IMAGE_ROW] float64: alpha x1 y1 x2 y2 h w l xc yc zc ry (KITTI's result-line order)
 *   on_image [B,top_k] uint8
 * A slot beyond det_counts[b], and a box with a non-finite field or h, w or l <= 0: twelve zeros, on_image 0.  Any
 * other detection that is off the image: x1 = y1 = x2 = y2 = 0, the other eight fields as computed, on_image 0.
 *
 * vn_eval_match_image: vn_eval_match with a third metric (VN_EVAL_BBOX: IoU of two axis-aligned 2D boxes, areas without
 * "+1", 0 when the union is <= 0) and the image-plane rules.  Takes what vn_eval_match takes, plus image_rows / on_image
 * (vn_boxes_to_image's outputs), gt_bbox [B,max_gt,4] and gt_alpha [B,max_gt] float64 (the label's x1 y1 x2 y2 and alpha),
 * dc_boxes [B,max_dc,4] float64 with dc_counts [B] (DontCare regions; 0 <= max_dc <= VN_EVAL_MAX_DC, both may be NULL
 * when max_dc == 0), min_height [n_diff] float64 ON THE DEVICE, and one threshold per metric.  Per frame, metric and
 * difficulty, vn_eval_match's walk with:
 *   - a detection with on_image == 0 or y2 - y1 < min_height[difficulty] is IGNORED (-1) before the walk and takes no
 *     ground truth;
 *   - after the walk, a detection left FP becomes IGNORED when area(det & D) / area(det) > 0.5 for a DontCare region D.
 *   status, matched_gt [B,3,n_diff,top_k]: as vn_eval_match's; axis 1: VN_EVAL_BEV, VN_EVAL_3D, VN_EVAL_BBOX
 *   similarity [B,n_diff,top_k] float64: (1 + cos(alpha_det - alpha_gt)) / 2 for a TP of the VN_EVAL_BBOX matching,
 *                                        else 0 (slots beyond the count included)
 *   iou_out    [B,3,top_k,max_gt] float64 or NULL;  workspace: vn_eval_match_workspace_bytes, the walk order as there
 * One workgroup per frame, one launch, no host synchronisation; limits and VN_EINVAL as vn_eval_match. */
#define VN_EVAL_BBOX 2
#define VN_EVAL_MAX_DC 64
#define VN_EVAL_IMAGE_ROW 12
int vn_boxes_to_image(const float *det_boxes, const int32_t *det_counts, const double *calib, const int32_t *image_hw,
                      int32_t B, int32_t top_k, double *rows, uint8_t *on_image, vnStream stream);
int vn_eval_match_image(const float *det_boxes, const float *det_scores, const int32_t *det_counts, const double *gt,
                        const int32_t *gt_counts, const uint8_t *gt_flags, const double *image_rows,
                        const uint8_t *on_image, const double *gt_bbox, const double *gt_alpha, const double *dc_boxes,
                        const int32_t *dc_counts, const double *min_height, int32_t B, int32_t top_k, int32_t max_gt,
                        int32_t max_dc, int32_t n_diff, double thr_bev, double thr_3d, double thr_bbox, int8_t *status,
                        int32_t *matched_gt, double *similarity, double *iou_out, void *workspace, size_t workspace_bytes,
                        vnStream stream);

/* ---- detection tail for evaluation (csrc/detect.hip; rules: DESIGN.md section 1c) ---------------------------
 * Extends the inference tail above (filter_boxes model.py:28-57, deltas_to_boxes_3d utils.py:476-489, utils.nms
 * utils.py:492-553), which lets only the NMS_POST_TOPK = 20 best candidates enter a stand-up-rectangle NMS
 * (utils.py:510), to the three steps an average precision needs: a pre-NMS top-K in the thousands, a greedy NMS on
 * stand-up rectangles or on the ROTATED footprints, a post-NMS cap.  vn_rpn_predict keeps the reference's behaviour.
 *
 * vn_rpn_select_decode (model.py:34, utils.py:476-489, 509-510): probs, deltas, anchors as for vn_rpn_predict.  Per
 * sample, of the M candidates with p >= score_thres (a NaN score is never one) the min(M, pre_top_k) largest by the
 * key (score, flat index) — equal scores: the LARGER flat index first, -0.0 == +0.0 — in descending key order:
 *   sel_boxes  [B,pre_top_k,7] float32: box j = flat delta elements 7j..7j+6 on anchor j, float64 arithmetic with a
 *                                       float32 expf, stored as float32 (exactly vn_rpn_predict's decoding)
 *   sel_scores [B,pre_top_k] float32, sel_idx [B,pre_top_k] int32 (flat index j), sel_counts [B] int32
 * Rows beyond sel_counts[b] are left untouched.  The keys are unique: the result does not depend on the order in
 * which the filter's atomics hand out slots.  Limits: 1 <= pre_top_k <= VN_DETECT_MAX_PRE, B * n_anchors < 2^28.
 *
 * vn_box_nms (utils.py:519-551 as an operation of its own): boxes [B,K,7] float32, row order = priority order;
 * counts [B] int32 read ON THE DEVICE (above K: K, below 0: 0).  Walk the rows in order; a row that is not suppressed
 * is kept; a kept row i suppresses every later row j with !(IoU(i,j) <= nms_thres); the walk stops once post_top_k
 * rows are kept.  keep_idx [B,post_top_k] int32 (row numbers, -1 beyond the count), keep_counts [B] int32.
 *   VN_NMS_STANDUP: vn_rpn_predict's arithmetic — float32 corners, float64 stand-up rectangles, areas without "+1";
 *                   a NaN IoU suppresses.
 *   VN_NMS_ROTATED: the BEV IoU of the detection scoring above (a float32 box is widened exactly; never NaN).  A row
 *                   with a non-finite field or h, w or l <= 0 is never kept and suppresses nothing.
 * Limits: 1 <= K <= VN_DETECT_MAX_PRE, 1 <= post_top_k <= VN_PREDICT_MAX_TOPK, nms_thres finite.
 *
 * vn_rpn_detect: vn_rpn_select_decode, vn_box_nms on its rows, and a gather of the kept rows into vn_rpn_predict's
 * output format: boxes [B,post_top_k,7], scores [B,post_top_k], counts [B]; rows beyond the count are not written.
 * Equal to the composition of the two operations exactly; with VN_NMS_STANDUP and pre_top_k == post_top_k
 * bit-identical to vn_rpn_predict; deterministic from run to run.
 *
 * All three: asynchronous on `stream`, no host synchronisation, one workgroup per sample after the filter pass.
 * VN_EINVAL for a size outside the limits, an unknown mode, a non-finite nms_thres or a null pointer (the workspace
 * queries return 0 for such sizes); VN_EWORKSPACE for a workspace smaller than the query's answer. */
#define VN_NMS_STANDUP 0
#define VN_NMS_ROTATED 1
#define VN_DETECT_MAX_PRE 4096
size_t vn_rpn_select_decode_workspace_bytes(int32_t B, int32_t n_anchors, int32_t pre_top_k);
int vn_rpn_select_decode(const float *probs, const float *deltas, const double *anchors, int32_t B, int32_t n_anchors,
                         float score_thres, int32_t pre_top_k, double anchor_h, float *sel_boxes, float *sel_scores,
                         int32_t *sel_idx, int32_t *sel_counts, void *workspace, size_t workspace_bytes, vnStream stream);
size_t vn_box_nms_workspace_bytes(int32_t B, int32_t K);
int vn_box_nms(const float *boxes, const int32_t *counts, int32_t B, int32_t K, int32_t mode, double nms_thres,
               int32_t post_top_k, int32_t *keep_idx, int32_t *keep_counts, void *workspace, size_t workspace_bytes,
               vnStream stream);
size_t vn_rpn_detect_workspace_bytes(int32_t B, int32_t n_anchors, int32_t pre_top_k);
int vn_rpn_detect(const float *probs, const float *deltas, const double *anchors, int32_t B, int32_t n_anchors,
                  float score_thres, int32_t pre_top_k, int32_t mode, double nms_thres, int32_t post_top_k,
                  double anchor_h, float *boxes, float *scores, int32_t *counts, void *workspace, size_t workspace_bytes,
                  vnStream stream);

/* The same two entry points with the layout in which the maps are read as an argument:
 *   VN_DETECT_FLAT: the reference's reshape without a permute, as above — candidate j is scored by flat element j of
 *                   probs[b] and decoded from flat elements 7j..7j+6 of deltas[b].  What the old entry points do; they call
 *                   these with VN_DETECT_FLAT and stay bit-identical.
 *   VN_DETECT_SITE: the layout the loss trains (vn_rpn_loss_*, vn_rpn_iou_loss) — anchor n = 2*s + a at site s = iy*W + ix
 *                   with rotation a is scored by probs[b,a,s] and decoded from deltas[b,7a+k,s], k = 0..6 (S = n_anchors/2
 *                   sites; n_anchors must be even, else VN_EINVAL).  Equal, bit for bit, to VN_DETECT_FLAT on contiguous
 *                   channels-last copies of the two maps.
 * Everything else is unchanged: the key (score, index n) and its tie rule, the decoding arithmetic, the NMS and the
 * gather, the limits, and the workspace sizes (the *_workspace_bytes queries above serve both layouts).  sel_idx is
 * the anchor index n in both layouts: the index of anchors, pos, targets and matched. */
#define VN_DETECT_FLAT 0
#define VN_DETECT_SITE 1
int vn_rpn_select_decode_layout(const float *probs, const float *deltas, const double *anchors, int32_t B, int32_t n_anchors,
                                float score_thres, int32_t pre_top_k, double anchor_h, float *sel_boxes, float *sel_scores,
                                int32_t *sel_idx, int32_t *sel_counts, void *workspace, size_t workspace_bytes, vnStream stream,
                                int32_t layout);
int vn_rpn_detect_layout(const float *probs, const float *deltas, const double *anchors, int32_t B, int32_t n_anchors,
                         float score_thres, int32_t pre_top_k, int32_t mode, double nms_thres, int32_t post_top_k,
                         double anchor_h, float *boxes, float *scores, int32_t *counts, void *workspace, size_t workspace_bytes,
                         vnStream stream, int32_t layout);

/* ---- anchor mask (SECOND's anchor_area_threshold; csrc/anchor_mask.hip; rules: DESIGN.md section 1k) -----------
 * An anchor over whose bird's-eye footprint the frame has (almost) no occupied voxel takes no part in the loss and can
 * never become a detection.  Every quantity is an integer: the outputs are exact, and bit-identical from run to run.
 *   coord  [K,4] int64 rows [b, d, h, w]: the batch's concatenated voxel coordinates.  occ[b,h,w] = the number of rows
 *          with that (b, h, w) — rows are counted, not de-duplicated; a row with b outside [0,B), h outside [0,H) or w
 *          outside [0,W) is ignored: neither counted nor written anywhere.  K == 0 is legal (coord may then be NULL):
 *          every count is 0.
 *   rects  [n_anchors,4] int32 = [w0, h0, w1, h1]: the INCLUSIVE cell rectangle of anchor n's footprint on the (H, W)
 *          grid, anchor order n = 2 * site + a — the order of pos.reshape(B, n_anchors).  Host work
 *          (voxelnet_amd/anchor_mask.py anchor_cell_rects: half-open footprint, edges within 1e-9 of a cell boundary
 *          snapped onto it, clipped to the grid).  w1 < w0 or h1 < h0: an empty rectangle, count 0.  A component outside
 *          the grid is clipped on the device.  16-byte aligned, else VN_EUNSUPPORTED.
 *   count  [B,n_anchors] int32, or NULL: sum of occ[b, h0..h1, w0..w1] — the whole rectangle.
 *   mask   [B,n_anchors] uint8: count > threshold (threshold >= 0; SECOND's value is 1).
 *   pos, neg [B,n_anchors] float32 IN PLACE, or both NULL: 0.0f is stored into both where mask == 0 (the anchor is
 *          ignored by the loss); a kept anchor's two floats are not written at all.
 *   workspace: vn_anchor_mask_workspace_bytes(B, H, W, n_anchors) bytes (0 for unsupported sizes: B, H, W or n_anchors
 *          <= 0, B * (H+1) * (W+1) or B * n_anchors >= 2^28).  The call clears whatever part of it it reads: its contents
 *          before the call do not matter.
 * A summed-area table (B, H+1, W+1) int32 is built in the workspace (an int32 atomicAdd per row of coord, a row pass, a
 * segmented column pass); the query is four reads per anchor for any anchor or voxel size.
 * VN_EINVAL, before anything is launched: a size outside the limits, K < 0 or K >= 2^31, threshold < 0, a NULL coord with
 * K > 0, a NULL rects / mask / workspace, exactly one of pos / neg NULL; VN_EWORKSPACE: workspace_bytes below the query's
 * answer.  Asynchronous on `stream`, no host synchronisation, no global state; integer atomics of an order-free sum only.
 *
 * vn_anchor_mask_probs: out = a COPY of probs (B, n_anchors floats per sample) in which a masked-out anchor's score is
 * +0.0f and every other element is bit-identical, in the layout the decode reads (VN_DETECT_FLAT: anchor n <-> flat element
 * n of probs[b];  VN_DETECT_SITE: anchor n = 2*s + a <-> probs[b,a,s], n_anchors even).  The detection tails above then
 * run unchanged on `out`; with score_thres <= 0 a score of 0 would be a candidate — the caller refuses that.  VN_EINVAL: a
 * NULL pointer, B or n_anchors <= 0, B * n_anchors >= 2^28, an unknown layout, or `out` overlapping `probs`. */
size_t vn_anchor_mask_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t n_anchors);
int vn_anchor_mask(const int64_t *coord, int64_t K, int32_t B, int32_t H, int32_t W, const int32_t *rects /*[n_anchors,4]*/,
                   int32_t n_anchors, int32_t threshold, uint8_t *mask, int32_t *count /*may be NULL*/,
                   float *pos /*in place; may be NULL*/, float *neg /*in place; NULL iff pos is*/, void *workspace,
                   size_t workspace_bytes, vnStream stream);
int vn_anchor_mask_probs(const float *probs, const uint8_t *mask, int32_t B, int32_t n_anchors, int32_t layout, float *out,
                         vnStream stream);

/* ---- test-time augmentation and box voting (csrc/tta.hip; rules: DESIGN.md section 1m) ---------------------------
 * What an evaluation does after the greedy NMS above has picked one box per cluster.  Both calls are asynchronous on
 * `stream`, never synchronise with the host, use no floating-point atomics and give the same bits from run to run.
 *
 * vn_pool_merge extends vn_rpn_select_decode: the candidate pools of V VIEWS of one batch (the frame flipped, rotated
 * and scaled by vn_augment_compose, each view decoded on its own) become one pool in one priority order, in the frame's
 * own coordinates — what vn_box_nms takes.
 *   boxes [V,B,K,7], scores [V,B,K] float32, counts [V,B] int32 (device): view v's rows k < min(max(counts[v,b], 0), K).
 *   views [V,3] float64 ON THE HOST, read during the call: fy (+1.0 or -1.0), angle, factor — the view's cloud was
 *         (x, y) -> (x, fy*y) -> turned by -angle -> times factor (augment.compose_affine's stages 2-4, no translation).
 *   Per sample the rows with a score that is not NaN come out in descending score (-0.0 == +0.0), equal scores with the
 *   SMALLER src = v*K + k first: out_boxes [B,V*K,7], out_scores [B,V*K], out_src [B,V*K] int32, out_counts [B] int32.
 *   Rows beyond out_counts[b] are left untouched.  Each box is mapped back by the exact inverse, float64 on the widened
 *   float32 fields with one float32 store:
 *       q[0..5] = (x', y', z', h', w', l') / factor;   c = cos(angle), s = sin(angle)   (host libm)
 *       X = q0*c - q1*s;   Y = q0*s + q1*c;   r = r' + angle;   out = (X, fy*Y, q2, q3, q4, q5, fy*r)   (r is not wrapped)
 *   A view with fy = +1, angle = 0 and factor = 1 copies its rows bit for bit.
 *   Limits: 1 <= V <= VN_TTA_MAX_VIEWS, B >= 1, K >= 1, V*K <= VN_DETECT_MAX_PRE; fy is +1 or -1, angle finite, factor
 *   finite and > 0.  One workgroup per sample: 64-bit keys (score bits | ~src) sorted in LDS, then a gather.
 *
 * vn_box_vote extends vn_box_nms: every kept row is replaced by the weighted mean of its cluster.
 *   boxes [B,K,7], scores [B,K], counts [B]: the pool vn_box_nms walked; keep_idx [B,P], keep_counts [B]: what it wrote.
 *   src [B,K] int32 or NULL, rows_per_view: row j belongs to view src[j] / rows_per_view (vn_pool_merge's out_src and K); a
 *   negative src or a view outside [0,V) takes no part in the view mean.  NULL: every row is view 0, and V must be 1.
 *   With n = clamp(counts[b], 0, K), m = clamp(keep_counts[b], 0, P), for each t < m, i = keep_idx[b,t]:
 *     an i outside [0,n) or a row i with a non-finite field or h, w, l <= 0 is skipped (vn_box_nms never writes one);
 *     members: row i (u_i = 1) and every other valid row j < n with u_j = IoU_bev(i,j) >= vote_thres (the pair function of
 *     vn_box_iou_rotated, float64 on the widened rows); weight w_j = s_j (VN_VOTE_W_SCORE) or s_j * u_j (VN_VOTE_W_SCORE_IOU);
 *     fields 0-5 = sum w_j q_jk / sum w_j;  yaw = r_i + sum w_j d_j / sum w_j with d_j = (r_j - r_i) - pi*floor((r_j - r_i)/pi + 0.5)
 *     (a member that points the other way counts as the same axis; the kept row's heading stays); float64 sums, one
 *     float32 store per field; when sum w_j is not > 0 the kept row is copied unchanged;
 *     score: the kept row's (VN_VOTE_S_KEEP), or the mean over the V views of the best member score of each view, 0 for
 *     a view without a member, summed in float64 in view order, divided by V, stored as float32 (VN_VOTE_S_VIEW_MEAN).
 *   out_boxes [B,P,7], out_scores [B,P], out_members [B,P] (the member count), out_counts [B]: the rows in descending
 *   output score, equal scores by t ascending (a NaN score behind every number); rows beyond out_counts[b] untouched.
 *   Limits: 1 <= B <= 65535, 1 <= K <= VN_DETECT_MAX_PRE, 1 <= P <= VN_PREDICT_MAX_TOPK, 1 <= V <= VN_TTA_MAX_VIEWS,
 *   vote_thres finite and > 0, src == NULL only with V == 1, else rows_per_view >= 1.
 *
 * Both: VN_EINVAL, before anything is launched, for a size or value outside the limits, an unknown mode or a null pointer
 * (src excepted); the workspace queries return 0 for sizes the call refuses; VN_EWORKSPACE for a smaller workspace. */
#define VN_TTA_MAX_VIEWS 8
#define VN_VOTE_W_SCORE 0        /* w_j = s_j */
#define VN_VOTE_W_SCORE_IOU 1    /* w_j = s_j * IoU(i,j) */
#define VN_VOTE_S_KEEP 0         /* the kept row's score */
#define VN_VOTE_S_VIEW_MEAN 1    /* mean over the V views of the best member score of that view (0 for a view without one) */
size_t vn_pool_merge_workspace_bytes(int32_t V, int32_t B, int32_t K);
int vn_pool_merge(const float *boxes /*[V,B,K,7]*/, const float *scores /*[V,B,K]*/, const int32_t *counts /*[V,B]*/,
                  const double *views /*[V,3], host*/, int32_t V, int32_t B, int32_t K, float *out_boxes /*[B,V*K,7]*/,
                  float *out_scores /*[B,V*K]*/, int32_t *out_src /*[B,V*K]*/, int32_t *out_counts /*[B]*/, void *workspace,
                  size_t workspace_bytes, vnStream stream);
size_t vn_box_vote_workspace_bytes(int32_t B, int32_t K, int32_t P, int32_t V);
int vn_box_vote(const float *boxes /*[B,K,7]*/, const float *scores /*[B,K]*/, const int32_t *counts /*[B]*/,
                const int32_t *src /*[B,K] or NULL*/, int32_t rows_per_view, const int32_t *keep_idx /*[B,P]*/,
                const int32_t *keep_counts /*[B]*/, int32_t B, int32_t K, int32_t P, int32_t V, double vote_thres,
                int32_t weight_mode, int32_t score_mode, float *out_boxes /*[B,P,7]*/, float *out_scores /*[B,P]*/,
                int32_t *out_members /*[B,P]*/, int32_t *out_counts /*[B]*/, void *workspace, size_t workspace_bytes,
                vnStream stream);

/* ---- Soft-NMS (csrc/soft_nms.hip; rules: DESIGN.md section 1n; Bodla et al., 2017) ---------------------------------
 * What vn_box_nms does with a DECAY in place of the deletion: a picked row multiplies the working score of every row it
 * overlaps by a decreasing function of the overlap, and the walk goes on by the decayed scores.  Asynchronous on `stream`,
 * never synchronises with the host, no floating-point atomics, the same bits from run to run.
 *   boxes [B,K,7], scores [B,K] float32, counts [B] int32 (device): the rows j < n = min(max(counts[b], 0), K) of sample b.
 *   A row is ELIGIBLE iff no field is non-finite, h, w, l > 0 (vn_box_iou_rotated's validity) and its score is finite; an
 *   ineligible row is never kept and decays nothing.  Working score w_j = (double)scores[j].  Repeat:
 *     i = the eligible, not yet picked, not removed row of the largest w (compared as numbers: -0.0 == +0.0), equal w: the
 *         SMALLER row; stop if there is none or if not (w_i >= min_score);
 *     keep_idx[b,t] = i, keep_scores[b,t] = (float)w_i; stop if t + 1 == post_top_k (before any decay);
 *     every remaining row j, u = IoU(i,j) by the pair function of vn_box_iou_rotated on the widened rows — VN_SOFT_BEV its BEV
 *     value, VN_SOFT_3D its 3D value —, takes ONE update:
 *       VN_SOFT_HARD:     removed if not (u <= iou_thres)
 *       VN_SOFT_LINEAR:   w_j = w_j * (1.0 - u)                   if u > iou_thres
 *       VN_SOFT_GAUSSIAN: w_j = w_j * exp(-(u*u) / sigma)         if u > 0          (float64 exp)
 *     (a pair whose centres are further apart than the two half-diagonals together has u = 0 exactly and is skipped unclipped).
 *   keep_idx [B,P] int32: -1 past the count; keep_scores [B,P] float32: 0 past the count; keep_counts [B] int32.  For
 *   non-negative input scores keep_scores does not increase along t.  A row's product is formed in pick order.
 *   VN_SOFT_HARD with VN_SOFT_BEV on a pool whose scores do not increase along the rows (and min_score at or below them) IS
 *   vn_box_nms(VN_NMS_ROTATED, nms_thres = iou_thres): the same keep_idx and keep_counts.
 *   Limits: B >= 1, 1 <= K <= VN_DETECT_MAX_PRE, 1 <= post_top_k <= VN_PREDICT_MAX_TOPK, a known method and metric, iou_thres
 *   finite in [0, 1], sigma finite and > 0 (read by VN_SOFT_GAUSSIAN only, checked always), min_score finite.  VN_EINVAL, before
 *   anything is launched, for anything else or a null pointer; the workspace query returns 0 for sizes the call refuses;
 *   VN_EWORKSPACE for a smaller workspace. */
#define VN_SOFT_HARD 0        /* the greedy rule: a row with IoU above iou_thres is removed */
#define VN_SOFT_LINEAR 1      /* w *= 1 - IoU above iou_thres */
#define VN_SOFT_GAUSSIAN 2    /* w *= exp(-IoU^2 / sigma) */
#define VN_SOFT_BEV 0
#define VN_SOFT_3D 1
size_t vn_box_soft_nms_workspace_bytes(int32_t B, int32_t K);
int vn_box_soft_nms(const float *boxes /*[B,K,7]*/, const float *scores /*[B,K]*/, const int32_t *counts /*[B]*/, int32_t B, int32_t K,
                    int32_t method, int32_t metric, double iou_thres, double sigma, double min_score, int32_t post_top_k,
                    int32_t *keep_idx /*[B,P]*/, float *keep_scores /*[B,P]*/, int32_t *keep_counts /*[B]*/, void *workspace,
                    size_t workspace_bytes, vnStream stream);

#ifdef __cplusplus
}
#endif
#endif /* VOXELNET_HIP_H */
