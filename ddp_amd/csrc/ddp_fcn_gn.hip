// ddp_fcn_gn.hip - the apply pass of a GroupNorm ConvWithTimeModule of FCNHeadWithTime (include/ddp_mi355x.h, ddp_fcn_conv with
// bn_w / bn_b set and bn_mean / bn_var NULL; decode_heads/fcn_head_with_time.py:205-225 with norm_cfg GN(32)) (gfx950, wave64).
//
// The statistics of GroupNorm depend on the activations, so norm x FiLM cannot be folded into the weights as the eval-mode BatchNorm
// is: the 3x3 convolution runs with its plain weights (stream GEMM, bias = conv bias, no activation; its epilogue or
// launch_gn_stats_blk leaves {mean, rstd} per (map, group)), and this ONE streaming pass turns the convolution's result, in place,
// into the next convolution's operand:
//   y[m][c] = ReLU( x[m][c] * a[map][c] + b[map][c] )
//   a = rstd * gamma * (1 + s)        b = (beta - mean * rstd * gamma) * (1 + s) + t        (s | t) = the conv's FiLM vector (or 0 | 0)
// ONE folding function (gn_film_fold) and ONE apply (gn_film_apply) with the fused multiply-adds spelled out serve every path, so
// the bits do not depend on which path an element takes or on what the compiler contracts where.
//
// Layout: fp32 fragment-major ("blk", ddp_kernels.hip): per 32-token group 64 pieces (4 channels) x 32 tokens x 16 B.  A block owns
// GF_GROUPS consecutive groups; thread = (piece % 8, token), so a wave's 64 lanes read and write 1 KiB contiguous with 16-byte
// accesses, eight loads in flight per lane.  The block folds (a | b) of the first two maps it touches into LDS once (256 threads =
// 256 channels; 4 KiB); a wave reads them back as two broadcast 16-byte rows (its two pieces).  Tokens of a third or later map in
// the same block - only maps of fewer than 64 tokens - fold their four channels in registers from the same inputs.  Padding rows of the
// last group (m >= rows) are neither read nor written.  No scratch.
#include "ddp_internal.h"

namespace ddp {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int GF_GROUPS = 4;     // 32-token groups per block (128 KiB read + written)
constexpr int GF_MAPS = 2;       // maps whose affine a block keeps in LDS

__device__ __forceinline__ void gn_film_fold(float mean, float rstd, float ga, float be, float s, float t, float& a, float& b) {
  const float n = rstd * ga, f = s + 1.0f;
  a = n * f;
  b = __fmaf_rn(__fmaf_rn(-mean, n, be), f, t);
}
__device__ __forceinline__ float gn_film_apply(float x, float a, float b) { return fmaxf(__fmaf_rn(x, a, b), 0.f); }

// y (rows, 256) blk in place; stats (maps, 32) {mean, rstd}; gamma, beta (256); film (512) scale | shift or nullptr; N tokens per map
__global__ void __launch_bounds__(256) k_gn_film_relu_blk(float* y, const float* __restrict__ stats, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, const float* __restrict__ film, int N,
                                                           int rows) {
  __shared__ __attribute__((aligned(16))) float aff[GF_MAPS][2][256];      // [map slot][a | b][channel]
  const int tid = threadIdx.x;
  const int m0 = blockIdx.x * (GF_GROUPS * 32);
  const int m_last = min(m0 + GF_GROUPS * 32, rows) - 1;
  const int b0 = m0 / N;
  const int nb = min(m_last / N - b0 + 1, GF_MAPS);
  {
    const int c = tid;
    const float ga = gamma[c], be = beta[c];
    const float s = film ? film[c] : 0.f, t = film ? film[256 + c] : 0.f;
    for (int k = 0; k < nb; ++k) {
      const float* sp = stats + (size_t(b0 + k) * 32 + (c >> 3)) * 2;
      float a, b;
      gn_film_fold(sp[0], sp[1], ga, be, s, t, a, b);
      aff[k][0][c] = a;
      aff[k][1][c] = b;
    }
  }
  __syncthreads();
  const int ml = tid & 31, pl = tid >> 5;
#pragma unroll 1
  for (int gl = 0; gl < GF_GROUPS; ++gl) {
    const int m = m0 + gl * 32 + ml;
    if (m >= rows) continue;
    const int k = m / N - b0;
    float* base = y + (size_t(m0 >> 5) + gl) * 8192 + pl * 128 + ml * 4;
    f32x4 v[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) v[it] = *reinterpret_cast<const f32x4*>(base + it * 1024);
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int c = (it * 8 + pl) * 4;
      f32x4 a, b;
      if (k < GF_MAPS) {
        a = *reinterpret_cast<const f32x4*>(&aff[k][0][c]);
        b = *reinterpret_cast<const f32x4*>(&aff[k][1][c]);
      } else {
        const float* sp = stats + (size_t(b0 + k) * 32 + (c >> 3)) * 2;
        const float mean = sp[0], rstd = sp[1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float ae, be;
          gn_film_fold(mean, rstd, gamma[c + e], beta[c + e], film ? film[c + e] : 0.f, film ? film[256 + c + e] : 0.f, ae, be);
          a[e] = ae;
          b[e] = be;
        }
      }
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = gn_film_apply(v[it][e], a[e], b[e]);
      *reinterpret_cast<f32x4*>(base + it * 1024) = o;
    }
  }
}

}  // namespace

int launch_gn_film_relu_blk(float* y_blk, const float* stats, const float* gamma, const float* beta, const float* film, int B, int N,
                            hipStream_t st) {
  if (B <= 0 || N <= 0) return DDP_OK;
  const long rows = long(B) * N;
  if (rows >> 31) {
    set_error("k_gn_film_relu_blk: %d maps of %d tokens are out of range", B, N);
    return DDP_E_BADCFG;
  }
  const long blocks = (rows + GF_GROUPS * 32 - 1) / (GF_GROUPS * 32);
  hipLaunchKernelGGL(k_gn_film_relu_blk, dim3(unsigned(blocks)), dim3(256), 0, st, y_blk, stats, gamma, beta, film, N, int(rows));
  return check_launch("k_gn_film_relu_blk");
}

}  // namespace ddp
