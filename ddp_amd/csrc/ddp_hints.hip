// ddp_hints.hip - DDP_FLAG_X0_HINTS (include/ddp_mi355x.h, "x0 hints"): the caller's per-image hint map (B, N) expanded into the
// per-row form the decision kernels read, once per ddp_sample.
//
// The x0 projection (segmentors/ddp.py:235-239; depth/depth/models/depther/ddp.py:240-246) is the loop's only feedback into the next
// step; where the caller knows the answer, that answer is projected instead of the model's prediction.  All r replicas of an image
// and all K steps share the image's map, so the rows are written once: row m = (b * r + rr) * N + n - the order of the x0 trace, of
// k_seg_update / the seg tails' token index and of the depth kernels' pixel index - takes map element b * N + n.  The "free"
// encodings are normalised here, so the consumers test ONE condition:
//   seg    any value >= num_classes -> 255            (consumer: f < num_classes ? f : its own argmax)
//   depth  0, negative, NaN, +-inf  -> 0.0f           (consumer: f > 0 ? f : its own prediction)
// Byte-streaming: one thread per 4 consecutive rows, one 4-byte (seg) / 16-byte (depth) store each; the row buffers are carved in
// whole 256-byte granules, so the last store may run into the padding behind row M - 1 but never out of the buffer.
#include "ddp_internal.h"

namespace ddp {
namespace {

// rows = B * r * N; rN = r * N.  (rows < 2^31: validate()'s token limit)
__global__ void __launch_bounds__(256) k_hint_rows_seg(const unsigned char* __restrict__ map, unsigned* __restrict__ rows4,
                                                       unsigned N, unsigned rN, unsigned rows, unsigned num_classes) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned m0 = t * 4u;
  if (m0 >= rows) return;
  unsigned word = 0;
#pragma unroll
  for (unsigned e = 0; e < 4; ++e) {
    const unsigned m = m0 + e;
    unsigned v = 255u;
    if (m < rows) {
      const unsigned b = m / rN, n = m % N;          // (m - b rN) % N == m % N: rN is a multiple of N
      v = map[size_t(b) * N + n];
      if (v >= num_classes) v = 255u;
    }
    word |= v << (8u * e);
  }
  rows4[t] = word;
}

__global__ void __launch_bounds__(256) k_hint_rows_depth(const float* __restrict__ map, float4* __restrict__ rows4, unsigned N,
                                                         unsigned rN, unsigned rows) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned m0 = t * 4u;
  if (m0 >= rows) return;
  float v[4];
#pragma unroll
  for (unsigned e = 0; e < 4; ++e) {
    const unsigned m = m0 + e;
    float x = 0.f;
    if (m < rows) {
      const unsigned b = m / rN, n = m % N;
      x = map[size_t(b) * N + n];
    }
    v[e] = (x > 0.f && x <= 3.402823466e+38f) ? x : 0.f;   // (NaN fails both comparisons; +inf the second)
  }
  rows4[t] = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace

int launch_hint_rows(const void* map, void* rows, int task, int B, int r, int N, int num_classes, hipStream_t st) {
  if (B <= 0 || r <= 0 || N <= 0) return DDP_OK;
  const size_t M = size_t(B) * r * N;
  if (M >> 31) {
    set_error("k_hint_rows: %d x %d maps of %d tokens are out of range", B, r, N);
    return DDP_E_BADCFG;
  }
  const unsigned threads = unsigned((M + 3) / 4), grid = (threads + 255u) / 256u;
  if (task == DDP_TASK_SEG) {
    hipLaunchKernelGGL(k_hint_rows_seg, dim3(grid), dim3(256), 0, st, static_cast<const unsigned char*>(map),
                       static_cast<unsigned*>(rows), unsigned(N), unsigned(r) * unsigned(N), unsigned(M), unsigned(num_classes));
    return check_launch("k_hint_rows_seg");
  }
  hipLaunchKernelGGL(k_hint_rows_depth, dim3(grid), dim3(256), 0, st, static_cast<const float*>(map), static_cast<float4*>(rows),
                     unsigned(N), unsigned(r) * unsigned(N), unsigned(M));
  return check_launch("k_hint_rows_depth");
}

}  // namespace ddp
