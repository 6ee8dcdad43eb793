/* ddp_eval_mi355x.h - C ABI of libddp_eval.so: the per-image `pre_eval` statistics of the reference's test protocol, reduced
 * on the MI355X (gfx950) next to the epilogue that wrote the map.  A library of its own: no part of the sampler ABI
 * (ddp_mi355x.h), not linked into libddp_mi355x.so.
 *
 * What it restates:
 *   seg    segmentation/mmseg/core/evaluation/metrics.py:66-87 `intersect_and_union` (label_map empty, as custom.py:311 passes it)
 *   depth  depth/depth/core/evaluation/metrics.py:7-44 `metrics` / `calculate`, with the Garg / Eigen rectangle of
 *          depth/depth/datasets/kitti.py:237-254 given by the caller
 *   bev    bev/mmdet3d/datasets/nuscenes_dataset.py:506-514 (tp / fp / fn per class and threshold)
 *
 * Conventions (those of ddp_mi355x.h)
 *  - plain C.  Every pointer named `d_*` is a DEVICE pointer to a contiguous array; the caller owns every buffer, the output
 *    and the workspace included; the library never allocates or frees device memory.
 *  - `items` is a HOST array of small structs; they travel by value inside the launch.  At most DDP_EVAL_MAX_ITEMS per call;
 *    the items of one call may differ in size.
 *  - all work is enqueued on the `hipStream_t` passed as `void* stream` (0 = default stream); no host synchronisation; every
 *    entry point can be captured into a hipGraph.  One call = one launch per task (depth: two, the second one the fixed-order
 *    final pass), plus the memset of its counter block.
 *  - return value: DDP_EVAL_OK (0) or a negative DDP_EVAL_E_* code (the values of DDP_E_*); `ddp_eval_last_error()` gives a
 *    message (thread-local).  A refused call enqueues nothing.
 */
#ifndef DDP_EVAL_MI355X_H
#define DDP_EVAL_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the entry points declared here are exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define DDP_EVAL_ABI_VERSION 1
#define DDP_EVAL_MAX_ITEMS 64
#define DDP_EVAL_SEG_BINS 256    /* row length of the seg counter block, whatever num_classes is */
#define DDP_EVAL_DEPTH_COLS 16   /* row length of the depth sums */
#define DDP_EVAL_MAX_THRESHOLDS 16

enum { DDP_EVAL_OK = 0, DDP_EVAL_E_BADCFG = -1, DDP_EVAL_E_ALIGN = -2, DDP_EVAL_E_LAUNCH = -3, DDP_EVAL_E_NULL = -4 };

const char* ddp_eval_last_error(void);
int ddp_eval_abi_version(void);

/* ---- seg ---------------------------------------------------------------------------------------------------------------
 * Per pixel: l' = label; with reduce_zero_label l' = (label == 0 || label == 255) ? 255 : label - 1 (the uint8 arithmetic of
 * metrics.py:70-73).  A pixel with l' == ignore_index is masked.  For every other pixel
 *   counts[1][pred]++ if pred < K      (area_pred_label)
 *   counts[2][l']++   if l' < K        (area_label)
 *   counts[0][pred]++ if pred == l' and pred < K   (area_intersect)
 * (torch.histc drops values outside [0, K-1]; a label >= K that is not ignore_index still counts its pixel's prediction.)
 * d_counts is (n_items, 3, DDP_EVAL_SEG_BINS) uint32, zeroed by the call; bins >= K stay 0.  union = pred + label - intersect
 * is the host's.  Maps are flat: any h, w with 1 <= h*w < 2^31, any byte alignment (16-byte loads run when d_pred and d_label
 * share their alignment modulo 16, with a bytewise head and tail).  num_classes 2..256 (K = 1: torch.histc(min=0, max=0) falls
 * back to the data range - the reference defines no answer).  ignore_index outside 0..255 masks nothing. */
typedef struct ddp_eval_seg_item {
  const uint8_t* d_pred;  /* (h, w) */
  const uint8_t* d_label; /* (h, w) */
  int32_t h, w;
} ddp_eval_seg_item;

int ddp_eval_seg(const ddp_eval_seg_item* items, int n_items, int num_classes, int ignore_index, int reduce_zero_label,
                 uint32_t* d_counts, void* stream);

/* ---- depth -------------------------------------------------------------------------------------------------------------
 * A pixel (y, x) is valid iff y0 <= y < y1, x0 <= x < x1 and gt > min_depth && gt < max_depth (fp32).  Over the valid pixels,
 * with g = gt, p = pred, d_sums (n_items, DDP_EVAL_DEPTH_COLS) double holds
 *   [0] n   [1..3] #{max(g/p, p/g) < 1.25, < 1.5625, < 1.953125}  (fp32, correctly rounded division: numpy's float32 result)
 *   [4] sum |g-p|/g   [5] sum (g-p)^2   [6] sum |log10 g - log10 p|   [7] sum (ln g - ln p)^2   [8] sum (ln p - ln g)
 *   [9] sum (g-p)^2/g   [10..15] 0        (fp64 arithmetic on the fp32 inputs)
 * Nothing is special-cased: a non-positive prediction gives the NaN the reference gives.  Sums go through per-block partials
 * in the workspace and a fixed-order final pass - no floating-point atomics; an item's row depends on that item alone, bit
 * for bit, wherever it stands in the call.  d_workspace: ddp_eval_depth_workspace() bytes, 8-byte aligned. */
typedef struct ddp_eval_depth_item {
  const float* d_pred; /* (h, w) */
  const float* d_gt;   /* (h, w) */
  int32_t h, w;
  int32_t y0, y1, x0, x1; /* the evaluated rectangle, [y0,y1) x [x0,x1) inside the map; the whole map = no crop */
} ddp_eval_depth_item;

int ddp_eval_depth_workspace(const ddp_eval_depth_item* items, int n_items, size_t* bytes);
int ddp_eval_depth(const ddp_eval_depth_item* items, int n_items, float min_depth, float max_depth, double* d_sums,
                   void* d_workspace, void* stream);

/* ---- bev ---------------------------------------------------------------------------------------------------------------
 * label = (gt != 0), hit = (prob >= thresholds[t]) in fp32.  d_counts (n_items, num_classes, n_thr, 3) uint32, zeroed by the
 * call: [0] tp = #(hit & label), [1] fp = #(hit & !label), [2] fn = #(!hit & label).  `thresholds` is a HOST array of
 * n_thr <= DDP_EVAL_MAX_THRESHOLDS floats, in any order.  1 <= num_classes <= 65535, 1 <= n_pix < 2^31. */
typedef struct ddp_eval_bev_item {
  const float* d_prob;  /* (num_classes, n_pix) */
  const uint8_t* d_gt;  /* (num_classes, n_pix) */
} ddp_eval_bev_item;

int ddp_eval_bev(const ddp_eval_bev_item* items, int n_items, int num_classes, int n_pix, const float* thresholds, int n_thr,
                 uint32_t* d_counts, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DDP_EVAL_MI355X_H */
