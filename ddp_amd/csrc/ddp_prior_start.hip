// ddp_prior_start.hip - DDP_FLAG_PRIOR_START (include/ddp_mi355x.h, "prior start"): the map the loop's first step reads, formed from
// the caller's prior map and the call's start noise, once per ddp_sample (gfx950, wave64).
//
// forward_train noises a known map to a time t and asks the head to recover it (segmentors/ddp.py:149-165, depther/ddp.py:133-143,
// fusion_models/ddp.py); here the same arithmetic starts the sampling chain at steps[0] = t_start:
//   seg / bev   m0[b][rr][ch][n] = alpha * x0[b][ch][n] + sigma * eps[b][rr][ch][n]
//   depth       m0[b][rr][0][n]  = alpha * x0[b][n]     + eps[b][rr][0][n] / sigma        (ddp_step.sigma of depth = 1 / sqrt(1 - gamma))
// with x0 of the PRIOR MAP (B, N), shared by the r replicas of an image:
//   seg    uint8: row min(value, num_classes) of the x0 table ddp_prepare builds ((num_classes + 1, 256); the last row is the ignore
//          row, ddp.py:151)
//   bev    uint32 bit word: (sigmoid(mean_c E[bit c ? c + 1 : 0]) * 2 - 1) * bit_scale, the sum in class order as k_bev_update forms it
//   depth  fp32 metric depth: the x0 normalisation of k_depth_update with its clamp; 0, negative, NaN, +-inf -> x0 = 0
// ONE mixing function (prior_mix / prior_mix_depth) serves every writer, with the fused multiply-add spelled out, so that the bits do
// not depend on what the compiler contracts where.
//
// Streaming over (B, r, Cm, N) NCHW.  seg / bev: a block owns ONE slab of 32 channels and stages that slab of the table, rows x 32
// floats, in LDS once ([row][33]: ds_read_b32 banks are dword % 32, so the 64 pixels of a wave - same channel, their own rows - hit
// bank (row + ch) % 32: distinct rows mod 32 never collide, equal rows broadcast); a 151 x 256 table would not fit whole.  It then
// walks (image, 1024-pixel chunk) items: a thread owns 4 consecutive pixels, reads their prior once, and per channel of the slab forms
// x0 once for all r replicas.  Global traffic is 16-byte loads and stores along the pixel axis wherever the 4 pixels are whole and
// the plane offset is a multiple of 4 elements (always when N % 4 == 0); the rest - the tail of a plane, and the planes of an N that
// is no multiple of 4 which start off a 16-byte boundary - goes element by element.  Plain stores: the first step's head reads the map
// next, it should stay in the cache hierarchy.  eps may be the output buffer (DDP_FLAG_SEEDED_NOISE: mixed in place) - every element
// is read and written by the same thread.  No scratch.
#include <stdint.h>
#include "ddp_internal.h"

namespace ddp {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PS_CH = 32;        // channels per slab
constexpr int PS_LD = PS_CH + 1; // row stride of the slab in LDS (floats)
constexpr int PS_PIX = 1024;     // pixels per item: 256 threads x 4

__device__ __forceinline__ float prior_mix(float alpha, float x0, float sigma, float eps) { return __fmaf_rn(alpha, x0, sigma * eps); }
__device__ __forceinline__ float prior_mix_depth(float alpha, float x0, float sigma, float eps) { return __fmaf_rn(alpha, x0, eps / sigma); }

// 4 (cnt < 4: the first cnt) consecutive elements at element offset `at`: m0 = mix(x0, eps)
template <bool DEPTH>
__device__ __forceinline__ void mix_store4(const float* eps, float* out, size_t at, int cnt, const float (&x0)[4], float alpha,
                                           float sigma, int vec) {
  if (vec && cnt == 4 && (at & 3u) == 0) {
    const f32x4 e = *reinterpret_cast<const f32x4*>(eps + at);
    f32x4 m;
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] = DEPTH ? prior_mix_depth(alpha, x0[i], sigma, e[i]) : prior_mix(alpha, x0[i], sigma, e[i]);
    *reinterpret_cast<f32x4*>(out + at) = m;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < cnt) out[at + i] = DEPTH ? prior_mix_depth(alpha, x0[i], sigma, eps[at + i]) : prior_mix(alpha, x0[i], sigma, eps[at + i]);
  }
}

// seg (BEV = false): tab = the x0 table (Kc + 1, 256), prior uint8.  bev: tab = the embedding (Kc + 1, 256), prior uint32.
// grid (groups, 8 slabs); ROWS = the most rows a slab can hold
template <bool BEV, int ROWS>
__global__ void __launch_bounds__(256) k_prior_start_tab(const void* __restrict__ prior, const float* __restrict__ tab, const float* eps,
                                                         float* out, int r, int N, int Kc, unsigned chunks, unsigned items, float alpha,
                                                         float sigma, float bit_scale, int vec) {
  __shared__ float slab[ROWS * PS_LD];
  const int tid = threadIdx.x, ch0 = blockIdx.y * PS_CH;
  const int rows = min(Kc + 1, ROWS);
  for (int i = tid; i < rows * PS_CH; i += 256) slab[(i >> 5) * PS_LD + (i & 31)] = tab[size_t(i >> 5) * 256 + ch0 + (i & 31)];
  __syncthreads();
  for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
    const unsigned b = item / chunks;
    const int n0 = int(item - b * chunks) * PS_PIX + tid * 4;
    if (n0 >= N) continue;
    const int cnt = min(4, N - n0);
    unsigned pv[4] = {0u, 0u, 0u, 0u};
    if constexpr (BEV) {
      const unsigned* p = static_cast<const unsigned*>(prior) + size_t(b) * N + n0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) pv[e] = p[e];
    } else {
      const unsigned char* p = static_cast<const unsigned char*>(prior) + size_t(b) * N + n0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) pv[e] = min(unsigned(p[e]), unsigned(Kc)) * PS_LD;     // (any value >= num_classes: the ignore row)
    }
    for (int c = 0; c < PS_CH; ++c) {
      float x0[4];
      if constexpr (BEV) {
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < Kc; ++k) {
#pragma unroll
          for (int q = 0; q < 4; ++q) e[q] += slab[(((pv[q] >> k) & 1u) ? k + 1 : 0) * PS_LD + c];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) x0[q] = (sigmoidf_(e[q] / float(Kc)) * 2.0f - 1.0f) * bit_scale;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) x0[q] = slab[pv[q] + c];
      }
      for (int rr = 0; rr < r; ++rr) {
        const size_t at = ((size_t(b) * r + rr) * 256 + ch0 + c) * size_t(N) + n0;
        mix_store4<false>(eps, out, at, cnt, x0, alpha, sigma, vec);
      }
    }
  }
}

// depth: Cm = 1, no table.  One thread per 4 consecutive pixels of one image, all r replicas
__global__ void __launch_bounds__(256) k_prior_start_depth(const float* __restrict__ prior, const float* eps, float* out, int r, int N,
                                                           unsigned chunks, unsigned items, float alpha, float sigma, float d_min,
                                                           float d_max, float bit_scale, int vec) {
  const unsigned item = blockIdx.x;
  if (item >= items) return;
  const unsigned b = item / chunks;
  const int n0 = int(item - b * chunks) * PS_PIX + int(threadIdx.x) * 4;
  if (n0 >= N) return;
  const int cnt = min(4, N - n0);
  float x0[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (e >= cnt) continue;
    const float d = prior[size_t(b) * N + n0 + e];
    if (d > 0.f && d <= 3.402823466e+38f) {                  // (NaN fails both comparisons; +inf the second)
      float x = (d - d_min) / (d_max - d_min);
      x = (x * 2.0f - 1.0f) * bit_scale;
      x0[e] = fminf(fmaxf(x, -bit_scale), bit_scale);
    }
  }
  for (int rr = 0; rr < r; ++rr) mix_store4<true>(eps, out, (size_t(b) * r + rr) * size_t(N) + n0, cnt, x0, alpha, sigma, vec);
}

}  // namespace

int launch_prior_start(const PriorStartArgs& a, hipStream_t st) {
  if (a.B <= 0 || a.r <= 0 || a.N <= 0) return DDP_OK;
  const size_t chunks = (size_t(a.N) + PS_PIX - 1) / PS_PIX, items = chunks * size_t(a.B);
  if (items >> 31) {
    set_error("k_prior_start: %d maps of %d tokens are out of range", a.B, a.N);
    return DDP_E_BADCFG;
  }
  // 16-byte accesses need 16-byte aligned tensors (the workspace buffers are; a caller's noise may be a view at any element)
  const int vec = ((reinterpret_cast<uintptr_t>(a.eps) | reinterpret_cast<uintptr_t>(a.out)) & 15u) == 0;
  if (a.task == DDP_TASK_DEPTH) {
    hipLaunchKernelGGL(k_prior_start_depth, dim3(unsigned(items)), dim3(256), 0, st, static_cast<const float*>(a.prior), a.eps, a.out,
                       a.r, a.N, unsigned(chunks), unsigned(items), a.alpha, a.sigma, a.min_depth, a.max_depth, a.bit_scale, vec);
    return check_launch("k_prior_start_depth");
  }
  if (a.num_classes < 1 || a.num_classes > (a.task == DDP_TASK_BEV ? 32 : 256)) {
    set_error("k_prior_start: num_classes %d out of range", a.num_classes);
    return DDP_E_BADCFG;
  }
  // each block stages its slab once: about 4 blocks per CU and slab, the items shared out between them
  const size_t want = size_t(cu_count()) * 4 / 8;
  const unsigned groups = unsigned(items < want ? items : (want ? want : 1));
  if (a.task == DDP_TASK_BEV) {
    hipLaunchKernelGGL((k_prior_start_tab<true, 33>), dim3(groups, 256 / PS_CH), dim3(256), 0, st, a.prior, a.table, a.eps, a.out, a.r,
                       a.N, a.num_classes, unsigned(chunks), unsigned(items), a.alpha, a.sigma, a.bit_scale, vec);
    return check_launch("k_prior_start_bev");
  }
  hipLaunchKernelGGL((k_prior_start_tab<false, 257>), dim3(groups, 256 / PS_CH), dim3(256), 0, st, a.prior, a.table, a.eps, a.out, a.r,
                     a.N, a.num_classes, unsigned(chunks), unsigned(items), a.alpha, a.sigma, a.bit_scale, vec);
  return check_launch("k_prior_start_seg");
}

}  // namespace ddp
