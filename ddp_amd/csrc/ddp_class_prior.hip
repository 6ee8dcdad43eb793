// ddp_class_prior.hip - DDP_FLAG_CLASS_PRIOR (include/ddp_mi355x.h, "class prior"): the caller's per-image class prior table (B, 256)
// normalised into the per-image vectors the seg decision kernels read, once per ddp_sample.
//
// The class a step decides on is what the loop feeds back (segmentors/ddp.py:235-239), so image-level knowledge about the classes has
// to act on the conv_seg scores of EVERY step (decode_head.py:133), in front of the argmax: row b of the table is one more bias of
// conv_seg for the tokens of image b.  All r replicas and all K steps share the row, so the vectors are written once per call:
//   bias_rows[b][k]  = fl32(head_b[k] + p)   the accumulator start of conv_seg in the layer kernel's seg tails (k_layer MODE 1 / 4 / 6,
//                                            the layout of tail_bias / tail4_bias / seg_bias: the class index, zero padded to 256)
//   delta_rows[b][k] = p                     added by k_seg_update to the scores of the head GEMM, which keeps conv_seg's own bias
// with p = clamp(NaN -> 0, -1e30, 1e30) of table[b][k] for k < num_classes and both 0 beyond.  The clamp keeps an excluded class
// (-inf) finite: its score is about -1e30, its softmax term exp(-1e30 - max) is exactly 0 and no infinity reaches the bilinear
// epilogues.  One thread per (image, class): 256 threads per block, one block per image; every access is in [0, B * 256).
#include "ddp_internal.h"

namespace ddp {
namespace {

__global__ void __launch_bounds__(256) k_class_prior(const float* __restrict__ table, const float* __restrict__ head_b,
                                                     float* __restrict__ bias_rows, float* __restrict__ delta_rows, int num_classes) {
  const int k = threadIdx.x;
  const size_t i = size_t(blockIdx.x) * 256 + k;
  float p = 0.f, b = 0.f;
  if (k < num_classes) {
    p = prior_normalise(table[i]);
    b = head_b[k] + p;
  }
  bias_rows[i] = b;
  delta_rows[i] = p;
}

}  // namespace

int launch_class_prior(const float* table, const float* head_b, float* bias_rows, float* delta_rows, int B, int num_classes,
                       hipStream_t st) {
  if (B <= 0) return DDP_OK;
  if (num_classes < 1 || num_classes > 256) {
    set_error("k_class_prior: num_classes %d out of range", num_classes);
    return DDP_E_BADCFG;
  }
  hipLaunchKernelGGL(k_class_prior, dim3(unsigned(B)), dim3(256), 0, st, table, head_b, bias_rows, delta_rows, num_classes);
  return check_launch("k_class_prior");
}

}  // namespace ddp
