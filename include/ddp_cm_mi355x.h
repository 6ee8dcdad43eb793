/* ddp_cm_mi355x.h - C ABI of libddp_cm.so: the K x K confusion matrix of the reference's
 * segmentation/tools/confusion_matrix.py:46-68 (`calculate_confusion_matrix`), accumulated on the MI355X (gfx950) from the class
 * maps where the epilogue wrote them.  A library of its own: no part of the sampler ABI (ddp_mi355x.h) or of the evaluation
 * library (ddp_eval_mi355x.h), linked into neither.
 *
 * Conventions (those of ddp_eval_mi355x.h)
 *  - plain C.  Every pointer named `d_*` is a DEVICE pointer to a contiguous array; the caller owns every buffer; the library never
 *    allocates or frees device memory.
 *  - `items` is a HOST array of small structs; they travel by value inside the launch.  At most DDP_CM_MAX_ITEMS per call; the
 *    items of one call may differ in size.
 *  - all work is enqueued on the `hipStream_t` passed as `void* stream` (0 = default stream); no host synchronisation; every
 *    entry point can be captured into a hipGraph.  One call = one launch, plus (accumulate = 0) the memsets of matrix and tally.
 *  - return value: DDP_CM_OK (0) or a negative DDP_CM_E_* code (the values of DDP_E_*); `ddp_cm_last_error()` gives a message
 *    (thread-local).  A refused call enqueues nothing.
 */
#ifndef DDP_CM_MI355X_H
#define DDP_CM_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the entry points declared here are exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define DDP_CM_ABI_VERSION 1
#define DDP_CM_MAX_ITEMS 64
#define DDP_CM_TALLY 4

enum { DDP_CM_OK = 0, DDP_CM_E_BADCFG = -1, DDP_CM_E_ALIGN = -2, DDP_CM_E_LAUNCH = -3, DDP_CM_E_NULL = -4 };

const char* ddp_cm_last_error(void);
int ddp_cm_abi_version(void);

/* The workspace of one ddp_cm_seg call with this num_classes (validated as there).  May return 0 bytes; d_workspace may then be
 * NULL. */
int ddp_cm_workspace(int num_classes, size_t* bytes);

/* ---- seg ---------------------------------------------------------------------------------------------------------------
 * Per pixel, K = num_classes:
 *   1. l' = label; with reduce_zero_label l' = (label == 0 || label == 255) ? 255 : label - 1 (the uint8 rule of ddp_eval_seg, so
 *      one loader of ground truth feeds both libraries).
 *   2. l' == ignore_index:  the pixel is masked,                 tally[1]++.  ignore_index outside 0..255 masks nothing.
 *   3. otherwise l' >= K:   the pixel is dropped,                tally[2]++   (the tool's reshape fails on such a label);
 *      otherwise pred >= K: the pixel is dropped,                tally[3]++   (the tool counts it in another row's bin);
 *      otherwise            matrix[l'][pred]++                                (rows: ground truth, columns: prediction -
 *                                                                              the tool's `n * gt + res`).
 *   tally[0]++ for every pixel, so tally[0] == tally[1] + tally[2] + tally[3] + sum(matrix) over the pixels of one call.
 * With reduce_zero_label = 0 and every label in {0..K-1, ignore_index}, every pred < K, this is calculate_confusion_matrix.
 *
 * The call adds the sum over ALL its items into ONE matrix, d_matrix (K, K) uint64 row-major, and one d_tally (DDP_CM_TALLY)
 * uint64 (NULL: no tally is kept).  accumulate = 0: both are zeroed first, by memsets on the same stream.  accumulate != 0: the
 * call adds to what they hold - the dataset-level accumulator; nothing is copied and nothing synchronises until the caller
 * reads them.  64-bit integer counters: the result is exact and does not depend on scheduling, on the order of the items or
 * on how a dataset is split into calls.
 *
 * Maps are flat: any h, w with 1 <= h*w < 2^31, any byte alignment (16-byte loads run when d_pred and d_label share their
 * alignment modulo 16, with a bytewise head and tail; otherwise the whole map goes bytewise).  num_classes 2..256.  d_matrix
 * and d_tally are 8-byte aligned.  Refusals: DDP_CM_E_BADCFG, DDP_CM_E_NULL, DDP_CM_E_ALIGN, before any launch. */
typedef struct ddp_cm_item {
  const uint8_t* d_pred;  /* (h, w) */
  const uint8_t* d_label; /* (h, w) */
  int32_t h, w;
} ddp_cm_item;

int ddp_cm_seg(const ddp_cm_item* items, int n_items, int num_classes, int ignore_index, int reduce_zero_label,
               int accumulate, uint64_t* d_matrix /* (K, K) */, uint64_t* d_tally /* (DDP_CM_TALLY) or NULL */,
               void* d_workspace, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DDP_CM_MI355X_H */
