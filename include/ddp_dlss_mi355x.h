/* ddp_dlss_mi355x.h - C ABI of libddp_dlss.so: what the reference's lidar-guided view transform (bev/mmdet3d/models/vtransforms/base.py
 * `BaseDepthTransform.forward`, depth_lss.py `DepthLSSTransform.get_cam_feats`) runs IN FRONT of the lift and pool of libddp_lss.so,
 * on the MI355X (gfx950): the projection of every lidar point into every camera, a deterministic scatter into the (B, N, 1, iH, iW)
 * depth image, and the first two `dtransform` stages in one kernel.  A library of its own: no part of the sampler ABI
 * (ddp_mi355x.h) nor of the evaluation, confusion-matrix or LSS libraries, linked into none of them.
 *
 * Three halves, each checkable on its own:
 *   project  (fp32 chain -> integers)  per (sample, camera, point) the pixel it falls on, or -1, and the clamped depth it carries
 *   scatter  (integers)                per pixel the candidate with the LARGEST POINT INDEX wins; exact, independent of atomic order
 *   stem     (fp32)                    conv 1x1 (1->8) + BN + ReLU + conv 5x5 stride 4 pad 2 (8->32) + BN + ReLU, eval-mode BN
 *
 * Conventions (those of ddp_lss_mi355x.h)
 *  - plain C.  Every pointer named `d_*` is a DEVICE pointer to a contiguous array, every pointer named `h_*` a HOST pointer; the
 *    caller owns every buffer; the library never allocates or frees device memory.
 *  - all work is enqueued on the `hipStream_t` passed as `void* stream` (0 = default stream); no host synchronisation; every
 *    entry point can be captured into a hipGraph (the host arrays are read during the call, the device pointers they hold are baked
 *    into the launches).
 *  - return value: DDP_DLSS_OK (0) or a negative DDP_DLSS_E_* code (the values of DDP_E_*); `ddp_dlss_last_error()` gives a message
 *    (thread-local).  A refused call enqueues nothing.
 *  - nothing depends on the arrival order of an atomic: two runs leave the same bytes in the tables, the image and the stem output,
 *    and a batched call equals per-sample calls.
 */
#ifndef DDP_DLSS_MI355X_H
#define DDP_DLSS_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the entry points declared here are exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define DDP_DLSS_ABI_VERSION 1
#define DDP_DLSS_WS_ALIGN 256
#define DDP_DLSS_STEM_MID 8       /* channels of the first dtransform convolution */
#define DDP_DLSS_STEM_OUT 32      /* channels of the second */
#define DDP_DLSS_STEM_FOLDED 6448 /* floats of the folded stem parameters: 8 + 8 + 25 * 8 * 32 + 32 */

enum { DDP_DLSS_OK = 0, DDP_DLSS_E_BADCFG = -1, DDP_DLSS_E_ALIGN = -2, DDP_DLSS_E_LAUNCH = -3, DDP_DLSS_E_NULL = -4 };

/* B samples of N cameras with iH x iW images; `pmax` is the row count the tables reserve per sample, at least every sample's point
 * count (0 is allowed: a batch without a point). */
typedef struct ddp_dlss_cfg {
  int32_t batch, cams, image_h, image_w, pmax;
} ddp_dlss_cfg;

/* The `dtransform` parameters as the state dict holds them, all DEVICE fp32: conv weights and biases, BatchNorm weight (gamma), bias
 * (beta), running_mean, running_var, and the two eps of the BatchNorm modules.  The library folds them itself (a launch of its own
 * in front of the stem kernel): scale = gamma / sqrt(var + eps), every division and square root correctly rounded. */
typedef struct ddp_dlss_stem_params {
  const float* d_conv1_weight; /* dtransform.0.weight (8, 1, 1, 1) */
  const float* d_conv1_bias;   /* dtransform.0.bias (8) */
  const float* d_bn1_weight;   /* dtransform.1.weight, .bias, .running_mean, .running_var (8 each) */
  const float* d_bn1_bias;
  const float* d_bn1_mean;
  const float* d_bn1_var;
  const float* d_conv2_weight; /* dtransform.3.weight (32, 8, 5, 5) */
  const float* d_conv2_bias;   /* dtransform.3.bias (32) */
  const float* d_bn2_weight;   /* dtransform.4.* (32 each) */
  const float* d_bn2_bias;
  const float* d_bn2_mean;
  const float* d_bn2_var;
  double bn1_eps, bn2_eps;
} ddp_dlss_stem_params;

const char* ddp_dlss_last_error(void);
int ddp_dlss_abi_version(void);

/* Limits, refused with DDP_DLSS_E_BADCFG before any launch: batch, cams, image_h, image_w >= 1; pmax >= 0; image_h*image_w < 2^31;
 * pmax < 2^31 (it is an int32: a negative value is what a larger one looks like); B*N*image_h*image_w < 2^31 and B*N*pmax < 2^31
 * (the tables and the image are indexed with 32-bit integers).  A NULL pointer is DDP_DLSS_E_NULL; d_workspace not
 * DDP_DLSS_WS_ALIGN-byte aligned, or any other pointer not 4-byte aligned, is DDP_DLSS_E_ALIGN.
 *
 * The workspace, with T = B*N*pmax table entries, X = B*N*iH*iW pixels and r(n) = n rounded up to 256 bytes:
 *   r(4T) pixel table + r(4T) depth table + r(4X) winner image + r(4 * 6448) folded stem parameters.
 * It carries the tables from ddp_dlss_project to ddp_dlss_scatter; nothing else survives a call, and no call reads what it did not
 * write. */
int ddp_dlss_workspace(const ddp_dlss_cfg* cfg, size_t* bytes);

/* ---- project -----------------------------------------------------------------------------------------------------------
 * h_points: B device pointers (a host array) to the point rows of each sample, `stride` floats per row (>= 3: x, y, z first; the
 * reference's rows have 5), h_counts: B host row counts, 0 <= count <= pmax (a zero count needs no valid pointer).  The points are
 * only read.
 *   d_lidar  (B, 12) floats: inverse(lidar_aug[:3,:3]) 9 row-major, lidar_aug[:3,3] 3
 *   d_cam    (B*N, 24): lidar2image[:3,:3] 9, lidar2image[:3,3] 3, img_aug[:3,:3] 9, img_aug[:3,3] 3
 * One thread per (point, camera), fp32, one rounding per operation, no fused multiply-add, sums left to right:
 *   1. p - lidar_aug_trans              2. multiply by inverse(lidar_aug_rot)     3. multiply by lidar2image_rot, add its trans
 *   4. z = clamp(z, 1e-5, 1e5)          5. x / z, y / z (true divisions)          6. multiply (x, y, z) by img_aug_rot, add its trans
 *   7. (row, col) = (y, x)              8. on the image iff 0 <= row < iH and 0 <= col < iW, compared as floats
 *   9. pixel = (int)row * iW + (int)col, truncated
 * A non-finite coordinate fails the comparisons of step 8 and drops the point.  Entry (b, n, p) of the pixel table (int32) is the
 * pixel or -1, of the depth table (fp32) the CLAMPED z of step 4 - the reference stores the clamped value through a view, so a point
 * behind a camera that still lands on the image carries 1e-5.  Entries p >= count are -1 and +0.0. */
int ddp_dlss_project(const ddp_dlss_cfg* cfg, const float* const* h_points, const int32_t* h_counts, int32_t stride,
                     const float* d_lidar, const float* d_cam, void* d_workspace, void* stream);

/* Where the two (B, N, pmax) tables lie in the workspace (host arithmetic only). */
int ddp_dlss_pixels(const ddp_dlss_cfg* cfg, void* d_workspace, const int32_t** d_pixels, const float** d_depths);

/* ---- scatter -----------------------------------------------------------------------------------------------------------
 * d_image is (B, N, 1, iH, iW) fp32.  Among the entries of one (b, n) that name a pixel, the one with the largest p wins (the
 * reference's indexed assignment on one CPU thread: the last point in point order).  A winner image of point indices, set to -1 by
 * the call itself, takes an integer atomic maximum per entry; a second pass writes depth_table[winner] or +0.0 to EVERY pixel: the
 * caller never clears the image.  Needs the tables of ddp_dlss_project in d_workspace, made with the same cfg. */
int ddp_dlss_scatter(const ddp_dlss_cfg* cfg, void* d_workspace, float* d_image, void* stream);

/* The same from a caller's (B, N, pmax) tables; a pixel outside [0, iH*iW) counts as -1.  The workspace holds the winner image. */
int ddp_dlss_scatter_from_tables(const ddp_dlss_cfg* cfg, const int32_t* d_pixels, const float* d_depths, void* d_workspace,
                                 float* d_image, void* stream);

/* ---- stem --------------------------------------------------------------------------------------------------------------
 * d_image (B*N, 1, iH, iW) -> d_out (B*N, 32, oH, oW) fp32 NCHW with oH = (iH - 1) / 4 + 1, oW = (iW - 1) / 4 + 1:
 *   a[c]   = relu(bn1(conv1(d)))[c]                      per pixel, recomputed per tap from a depth patch in LDS, never stored
 *   out[o] = relu(bn2(conv2(a)))[o]                      5 x 5, stride 4, zero padding 2 OF a: a tap outside the image adds 0
 * with eval-mode BatchNorm folded into the convolutions.  Every element of d_out is written.  `pmax` of cfg is not used beyond the
 * workspace layout. */
int ddp_dlss_stem(const ddp_dlss_cfg* cfg, const float* d_image, const ddp_dlss_stem_params* params, void* d_workspace, float* d_out,
                  void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DDP_DLSS_MI355X_H */
