// ddp_ddpm_chain.hip - DDP_FLAG_DDPM_CHAIN: the noise term of a ddpm step on the u chain (gfx950, wave64).
//
// The seg sampler's u chain carries the noisy map only as u = W_m . m (fp32 fragment-major, o.ubuf) and lets the step's tail
// (k_layer MODE 4 / 6) run u' = ua u + uc T[argmax].  The ddpm update (segmentors/ddp.py:274-283) adds std . eps to the map, which
// under W_m is std . (W_m eps): affine, but not a table row.  k_u_noise is the pre-pass that folds it in, in place,
//   U <- ua' U + std (E W_m^T),   ua' = ((1 - c) / alpha) alpha_next,
// after which the tail runs with (ua, uc) = (1, c alpha_next).  (Dividing the noise by ua' instead is not possible: ua' is 0 when
// c rounds to 1.)  One launch per noise-adding step.
//
// Arithmetic: fp32 operands on the exact-product fp32 MFMA (v_mfma_f32_32x32x2_f32, as gemm_f32.h): std . W_m eps is of the order of
// q itself, so a single bf16 product will not do.  The weight tile is the MFMA's A operand, so the 32 x 32 accumulator of (32
// channels) x (32 tokens) IS the fragment layout of U - ubuf + grp * 8192 + t * 1024 + g * 256 + lane * 4 + e, lane j + 32 h holding
// channel 32 t + 8 g + 4 h + e of token 32 grp + j - and the epilogue is one 16-byte load, four fmas and one 16-byte store per slot.
//
// Block = 8 waves; wave t owns channels [32 t, 32 t + 32) and keeps its 32 x 256 slice of W_m in 128 registers for the whole
// (persistent) launch.  A block walks 32-token groups blockIdx, + grid, ...: the group's 32 rows of E (token-major, 1 KiB each) are
// fetched with whole-row coalesced loads one group ahead, staged in LDS (row stride 260 floats: conflict-free 16-byte reads) and read
// by all eight waves as the B operand.  The 256 input channels are summed in the order (8 c + 4 kh + e): kh is the MFMA's two-deep
// k, e the four MFMAs of a 16-byte piece, c the 32 pieces of a row - the same order in every lane, block and launch.
// Rows >= M (the pad of the last group) are loaded from the clamped row M - 1 and replaced by zeros, so nothing is read past E's M
// rows and pad rows of U become ua' U.  Every element of U is read and written by exactly one lane of one block.
// Resources: 32.5 KiB of static LDS, < 256 registers (two waves per SIMD), no scratch (tests/test_ddpm_chain_host.py).
#include "ddp_internal.h"

namespace ddp {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int UN_THREADS = 512;
constexpr int UN_LD = 260;   // LDS row stride (floats)

__global__ void __launch_bounds__(UN_THREADS) k_u_noise(float* __restrict__ U, const float* __restrict__ E, const float* __restrict__ W,
                                                        int M, int groups, float ua, float sd) {
  __shared__ __attribute__((aligned(16))) float es[32 * UN_LD];
  const int tid = threadIdx.x, lane = tid & 63, t = tid >> 6, j = lane & 31, h = lane >> 5;
  // A operand: lane (j, h) holds W_m[32 t + j][8 c + 4 h + e]
  f32x4 w[32];
  {
    const float* wp = W + size_t(32 * t + j) * 256 + 4 * h;
#pragma unroll
    for (int c = 0; c < 32; ++c) w[c] = *reinterpret_cast<const f32x4*>(wp + 8 * c);
  }
  // staging: thread (srow, scol) moves rows srow + 8 i of the group, 16 bytes at column scol
  const int srow = tid >> 6, scol = (tid & 63) * 4;
  f32x4 pre[4];
  auto fetch = [&](int grp) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = grp * 32 + srow + 8 * i;
      const int mc = m < M ? m : M - 1;
      const f32x4 v = *reinterpret_cast<const f32x4*>(E + size_t(mc) * 256 + scol);
      pre[i] = m < M ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  int grp = blockIdx.x;
  if (grp < groups) fetch(grp);
  for (; grp < groups; grp += gridDim.x) {
    __syncthreads();                                   // the previous group's B reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>(es + (srow + 8 * i) * UN_LD + scol) = pre[i];
    __syncthreads();
    if (grp + int(gridDim.x) < groups) fetch(grp + int(gridDim.x));
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* ep = es + j * UN_LD + 4 * h;          // B operand: lane (j, h) holds E[32 grp + j][8 c + 4 h + e]
#pragma unroll
    for (int c = 0; c < 32; ++c) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(ep + 8 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[c][e], b[e], acc, 0, 0, 0);
    }
    float* up = U + size_t(grp) * 8192 + t * 1024 + lane * 4;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 u = *reinterpret_cast<const f32x4*>(up + g * 256);
#pragma unroll
      for (int e = 0; e < 4; ++e) u[e] = fmaf(sd, acc[4 * g + e], ua * u[e]);
      *reinterpret_cast<f32x4*>(up + g * 256) = u;
    }
  }
}

}  // namespace

int launch_u_noise(float* ubuf, const float* noise, const float* wm, int M, float ua, float std, hipStream_t st) {
  if (M <= 0) return DDP_OK;
  if (!ubuf || !noise || !wm) {
    set_error("k_u_noise: u, the step noise and W_m are all required");
    return DDP_E_NULL;
  }
  const int groups = (M + 31) / 32;
  const int n_cu = cu_count();
  const int grid = groups < n_cu ? groups : n_cu;
  hipLaunchKernelGGL(k_u_noise, dim3(grid), dim3(UN_THREADS), 0, st, ubuf, noise, wm, M, groups, ua, std);
  return check_launch("k_u_noise");
}

}  // namespace ddp
