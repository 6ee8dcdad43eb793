// ddp_step_record.hip - DDP_FLAG_STEP_RECORD: the bev step record and the step-disagreement map (gfx950, wave64).
//
// The record (K, B, r, H, W) is written where the per-step values already exist (csrc/ddp_api.hip): seg through the tails' x0_idx
// pointer, depth through k_depth_update's pred pointer; only bev needs a kernel of its own, which widens what the step's route
// left (the u chain's code byte, or the raw conv_seg logits of the separate kernels) to one uint32 bit word per head-grid token.
// k_step_disagreement then reduces the K * r records of a pixel against the output ddp_sample returned.  Both kernels are
// byte-streaming, one thread per token / pixel, consecutive threads on consecutive addresses; no LDS, no scratch.
#include <math.h>
#include "ddp_internal.h"

namespace ddp {
namespace {

// bev (fusion_models/ddp.py:290): rec[m] bit c = prob_c > threshold at head-grid token m (sigmoidf_ of ddp_internal.h: the one
// expression k_bev_update / k_bev_seg3 threshold, so the record holds the decisions those kernels fed back).  code != nullptr: the
// step's code byte (bit c as above, K_cls <= 8) - a widening copy; else logits (M, 32) raw conv_seg rows
__global__ void __launch_bounds__(256) k_bev_record(const unsigned char* __restrict__ code, const float* __restrict__ logits,
                                                    unsigned* __restrict__ rec, int num_classes, float threshold, int M) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= M) return;
  unsigned bits = 0;
  if (code) {
    bits = code[m];
  } else {
    const float* lg = logits + size_t(m) * 32;
    for (int k = 0; k < num_classes; ++k)
      if (sigmoidf_(lg[k]) > threshold) bits |= 1u << k;
  }
  rec[m] = bits;
}

// One thread per output pixel (b, n) walks the K * r records of the pixel: rec[(s * B * r + b * r + ri) * N + n].
//   seg   fraction of the records that differ from argmax_c out[b][c][n] (first maximum wins, as k_seg_postprocess)
//   bev   mean over records and classes of [bit_c != (out[b][c][n] > threshold)]
//   depth population standard deviation of the records, two passes in fp32
// A single record (K * r == 1) gives 0 by each definition.
__global__ void __launch_bounds__(256) k_step_disagreement(StepDisagreementArgs a) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= a.B * a.N) return;
  const int b = idx / a.N, n = idx - b * a.N;
  const size_t step_stride = size_t(a.B) * a.r * a.N;
  const size_t first = size_t(b) * a.r * a.N + n;
  const int count = a.K * a.r;
  float res;
  if (a.task == DDP_TASK_DEPTH) {
    const float* rec = static_cast<const float*>(a.rec) + first;
    float sum = 0.f;
    for (int s = 0; s < a.K; ++s)
      for (int ri = 0; ri < a.r; ++ri) sum += rec[s * step_stride + size_t(ri) * a.N];
    const float mean = sum / float(count);
    float ss = 0.f;
    for (int s = 0; s < a.K; ++s)
      for (int ri = 0; ri < a.r; ++ri) {
        const float d = rec[s * step_stride + size_t(ri) * a.N] - mean;
        ss = fmaf(d, d, ss);
      }
    res = sqrtf(ss / float(count));
  } else if (a.task == DDP_TASK_SEG) {
    const float* o = a.out + size_t(b) * a.num_classes * a.N + n;
    float best = o[0];
    int bi = 0;
    for (int c = 1; c < a.num_classes; ++c) {
      const float v = o[size_t(c) * a.N];
      if (v > best) {
        best = v;
        bi = c;
      }
    }
    const unsigned char* rec = static_cast<const unsigned char*>(a.rec) + first;
    int diff = 0;
    for (int s = 0; s < a.K; ++s)
      for (int ri = 0; ri < a.r; ++ri) diff += rec[s * step_stride + size_t(ri) * a.N] != bi;
    res = float(diff) / float(count);
  } else {
    const float* o = a.out + size_t(b) * a.num_classes * a.N + n;
    unsigned fin = 0;
    for (int c = 0; c < a.num_classes; ++c)
      if (o[size_t(c) * a.N] > a.threshold) fin |= 1u << c;
    const unsigned* rec = static_cast<const unsigned*>(a.rec) + first;
    int diff = 0;
    for (int s = 0; s < a.K; ++s)
      for (int ri = 0; ri < a.r; ++ri) diff += __popc(rec[s * step_stride + size_t(ri) * a.N] ^ fin);
    res = float(diff) / float(count * a.num_classes);
  }
  a.map[idx] = res;
}

}  // namespace

int launch_bev_record(const unsigned char* code, const float* logits, unsigned* rec, int num_classes, float threshold, int M,
                      hipStream_t st) {
  if (M <= 0) return DDP_OK;
  if (num_classes < 1 || num_classes > 32 || (code && num_classes > 8) || (!code && !logits)) {
    set_error("k_bev_record: unsupported call (%d classes, code byte %d)", num_classes, code ? 1 : 0);
    return DDP_E_BADCFG;
  }
  hipLaunchKernelGGL(k_bev_record, dim3((M + 255) / 256), dim3(256), 0, st, code, logits, rec, num_classes, threshold, M);
  return check_launch("k_bev_record");
}

int launch_step_disagreement(const StepDisagreementArgs& a, hipStream_t st) {
  const long total = long(a.B) * a.N;
  if (total <= 0) return DDP_OK;
  hipLaunchKernelGGL(k_step_disagreement, dim3(int((total + 255) / 256)), dim3(256), 0, st, a);
  return check_launch("k_step_disagreement");
}

}  // namespace ddp
