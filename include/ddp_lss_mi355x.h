/* ddp_lss_mi355x.h - C ABI of libddp_lss.so: the lift and pool of the reference's camera-only BEV view transform
 * (bev/mmdet3d/models/vtransforms/base.py `get_geometry` + `bev_pool`, lss.py `get_cam_feats`) on the MI355X (gfx950), without the
 * (B, N, D, fH, fW, C) volume.  A library of its own: no part of the sampler ABI (ddp_mi355x.h), of the evaluation library or of the
 * confusion-matrix library, linked into none of them.
 *
 * Two halves, each checkable exactly:
 *   plan  (integers)  which frustum point falls into which BEV cell: a rank table and, per cell, the ascending list of its points
 *   pool  (fp32)      out[cell, c] = sum over the cell's list, in list order, of softmax(depth)[p] * context[pixel(p), c]
 *
 * Conventions (those of ddp_cm_mi355x.h)
 *  - plain C.  Every pointer named `d_*` is a DEVICE pointer to a contiguous array; the caller owns every buffer; the library never
 *    allocates or frees device memory.
 *  - all work is enqueued on the `hipStream_t` passed as `void* stream` (0 = default stream); no host synchronisation; every
 *    entry point can be captured into a hipGraph.
 *  - return value: DDP_LSS_OK (0) or a negative DDP_LSS_E_* code (the values of DDP_E_*); `ddp_lss_last_error()` gives a message
 *    (thread-local).  A refused call enqueues nothing.
 *  - nothing depends on the arrival order of an atomic: a plan built twice holds the same bytes, a pooled output is bit-identical
 *    from run to run and between one batched call and per-sample calls.
 */
#ifndef DDP_LSS_MI355X_H
#define DDP_LSS_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the entry points declared here are exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define DDP_LSS_ABI_VERSION 1
#define DDP_LSS_MAX_CHANNELS 256
#define DDP_LSS_MAX_DEPTH_BINS 512
#define DDP_LSS_WS_ALIGN 256

enum { DDP_LSS_OK = 0, DDP_LSS_E_BADCFG = -1, DDP_LSS_E_ALIGN = -2, DDP_LSS_E_LAUNCH = -3, DDP_LSS_E_NULL = -4 };

/* The geometry of one LSSTransform.  The bounds are the (lo, hi, step) triples of the configuration as the doubles Python holds;
 * from them the library forms, as the reference does, dx = fp32(step), bx = fp32(lo + step / 2.0), the cell origin bx - dx / 2 in
 * fp32, and the depth of bin d, fp32(lo + d * step) evaluated in double (`torch.arange(*dbound, dtype=torch.float)`).
 * `nx` and `depth_bins` are GIVEN, not derived: the reference truncates a Python-float division (`torch.LongTensor([(hi - lo) /
 * step])`) and takes `len(torch.arange(*dbound))`; the caller evaluates those expressions where the reference does. */
typedef struct ddp_lss_cfg {
  int32_t batch, cams, depth_bins, feat_h, feat_w, channels; /* B, N, D, fH, fW, C */
  int32_t image_h, image_w;                                  /* iH, iW: xs = linspace(0, iW - 1, fW), ys = linspace(0, iH - 1, fH) */
  double dbound[3], xbound[3], ybound[3], zbound[3];
  int32_t nx[3];                                             /* cells along x, y, z */
} ddp_lss_cfg;

const char* ddp_lss_last_error(void);
int ddp_lss_abi_version(void);

/* Limits, refused with DDP_LSS_E_BADCFG before any launch: channels 1..256, depth_bins 1..512, every extent (batch, cams, feat_*,
 * image_*, nx[*]) >= 1, every step > 0 and finite, B*N*D*fH*fW < 2^31 and B*nz*nx0*nx1 < 2^31.  A NULL pointer is DDP_LSS_E_NULL;
 * d_workspace not DDP_LSS_WS_ALIGN-byte aligned, or any other pointer not 4-byte aligned, is DDP_LSS_E_ALIGN.
 *
 * The workspace, with P = B*N*D*fH*fW points, K = B*nz*nx0*nx1 cells, X = B*N*fH*fW pixels and r(n) = n rounded up to 256 bytes:
 *   r(4P) ranks + r(4(K+1)) offsets + r(4K) cursors + r(4 ceil(K/1024)) tile sums + r(4P) unsorted lists + r(4P) lists
 *   + r(4P) probabilities + r(4XC) rows.
 * It carries the plan from ddp_lss_plan* to ddp_lss_pool; nothing else survives a call, and no call reads what it did not write. */
int ddp_lss_workspace(const ddp_lss_cfg* cfg, size_t* bytes);

/* ---- plan --------------------------------------------------------------------------------------------------------------
 * Point p = (((b*N + n)*D + d)*fH + h)*fW + w is the frustum point (xs[w], ys[h], ds[d]).  In fp32, one rounding per operation and
 * no fused multiply-add (the chain of `get_geometry`):
 *   1. subtract post_trans         2. multiply by inverse(post_rot)      3. (x*z, y*z, z)       4. multiply by combine
 *   5. add camera2lidar_trans      6. multiply by extra_rot              7. add extra_trans
 * then per axis q = (g - (bx - dx/2)) / dx, a true fp32 division, and i = (int)q, truncated TOWARD ZERO as `.long()` does: a
 * coordinate in (-1, 0) lands in cell 0 and is kept.  A point is kept when 0 <= i < nx on all three axes; a non-finite coordinate
 * drops the point (the reference is undefined there).  rank = ((b*nz + iz)*nx0 + ix)*nx1 + iy, or -1 for a dropped point.
 *
 *   d_cam    (B*N, 24) floats per camera, row-major 3 x 3 matrices: inverse(post_rot) 9, post_trans 3,
 *            combine = camera2lidar_rot * inverse(intrinsics) 9, camera2lidar_trans 3
 *   d_extra  (B, 12): extra_rot 9, extra_trans 3
 * The plan is the rank table plus, per cell, the list of its points in ascending p. */
int ddp_lss_plan(const ddp_lss_cfg* cfg, const float* d_cam, const float* d_extra, void* d_workspace, void* stream);

/* The same plan from a caller's (P) int32 rank table; an entry outside [0, K) counts as -1 (and is stored as -1). */
int ddp_lss_plan_from_ranks(const ddp_lss_cfg* cfg, const int32_t* d_ranks, void* d_workspace, void* stream);

/* Where the plan's rank table lies in the workspace (host arithmetic only). */
int ddp_lss_ranks(const ddp_lss_cfg* cfg, void* d_workspace, const int32_t** d_ranks);

/* ---- pool --------------------------------------------------------------------------------------------------------------
 * d_depthnet_out is the (B*N, D + C, fH, fW) fp32 tensor the 1 x 1 `depthnet` convolution emits, unmodified: the softmax over the
 * first D channels (expf of the difference to the per-pixel maximum, over the sum) is part of this call.
 * d_out is (B, nz*C, nx0, nx1) fp32 NCHW, channel z*C + c: `torch.cat(x.unbind(dim=2), 1)` of base.py:161.  Every element is
 * written, zeros (+0.0) included; the caller never clears it.  Needs a plan in d_workspace made with the same cfg. */
int ddp_lss_pool(const ddp_lss_cfg* cfg, const float* d_depthnet_out, void* d_workspace, float* d_out, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DDP_LSS_MI355X_H */
