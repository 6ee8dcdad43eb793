// ddp_score_prior.hip - DDP_FLAG_SCORE_PRIOR (include/ddp_mi355x.h, "score prior"): the caller's per-pixel score prior map
// (B, num_classes, N), NCHW like d_out, normalised and transposed into the token-major rows the seg decision kernels read, once per
// ddp_sample.
//
// Soft knowledge that varies over the image (a cheaper model's logits, last frame's scores, a scribble with a strength, a region where
// some classes cannot occur) has to act where the class prior acts: on the conv_seg scores of EVERY step, in front of the argmax that
// is fed back (segmentors/ddp.py:235-239).  The readers are per token - a lane of the layer kernel's seg tails holds 32 classes of one
// token, a wave of k_seg_update one token - so they want the prior of a pixel as one contiguous row:
//   rows[b * N + n][k] = p(map[b][k][n])  for k < num_classes, 0 for num_classes <= k < KP,  KP = 64 * ceil(num_classes / 64)
// with p = prior_normalise (NaN -> 0, clamp to +-1e30: the class prior's rule, one __device__ function for both).  All r replicas and
// all K steps read the same rows.
//
// k_score_prior_rows: one block per (image, 64 pixels, 64 classes).  Lane = pixel on the way in - each of a wave's 16 class planes is
// one coalesced 256-byte read - and four consecutive classes of a pixel go to LDS as one 16-byte store; on the way out 16 lanes write
// the 64 classes of a pixel as one 256-byte line in 16-byte stores.  LDS tile (64 pixels, 68 floats): the 16-byte stores of 8
// consecutive pixels (one ds_write_b128 lane group; banks mod 32) start 4 banks apart, and a ds_read_b128 lane group (16 lanes of two
// pixels, banks mod 64; MI355X_MICROARCH "LDS") reads slot (pixel + c4) mod 16 = lane mod 16 with c4 = (lane - pixel) mod 16: sixteen
// different 16-byte slots.  No conflicts on either side.  Pixels >= N are not written and classes >= num_classes are written as 0;
// their loads are redirected to the last pixel / the last class, so every access is inside map (B * num_classes * N) and rows
// (B * N * KP).
#include "ddp_internal.h"

namespace ddp {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int SP_TILE = 64, SP_LD = 68;

__global__ void __launch_bounds__(256) k_score_prior_rows(const float* __restrict__ map, float* __restrict__ rows, int num_classes, int N,
                                                          int tiles_n, int chunks) {
  __shared__ __attribute__((aligned(16))) float tile[SP_TILE * SP_LD];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int kc = blockIdx.x % chunks, rest = blockIdx.x / chunks;
  const int n0 = (rest % tiles_n) * SP_TILE, b = rest / tiles_n;
  const int k0 = kc * 64;
  {
    // every load is issued - a pixel >= N reads pixel N - 1, a class >= num_classes the last class, both in range - so that the 16
    // loads of a lane are in flight together; what they returned is dropped below
    const int n = n0 + lane;
    const float* src = map + size_t(b) * num_classes * N + (n < N ? n : N - 1);
    float raw[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int k = k0 + wv * 16 + i;
      raw[i] = src[size_t(k < num_classes ? k : num_classes - 1) * N];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (n < N && k0 + wv * 16 + 4 * i + e < num_classes) ? prior_normalise(raw[4 * i + e]) : 0.f;
      *reinterpret_cast<f32x4*>(tile + lane * SP_LD + 16 * wv + 4 * i) = v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int px = wv * 16 + i * 4 + (lane >> 4);
    const int c4 = (lane - px) & 15;
    const f32x4 v = *reinterpret_cast<const f32x4*>(tile + px * SP_LD + 4 * c4);
    if (n0 + px < N) *reinterpret_cast<f32x4*>(rows + (size_t(b) * N + n0 + px) * (size_t(chunks) * 64) + k0 + 4 * c4) = v;
  }
}

}  // namespace

int launch_score_prior_rows(const float* map, float* rows, int B, int num_classes, int N, hipStream_t st) {
  if (B <= 0 || N <= 0) return DDP_OK;
  if (num_classes < 1 || num_classes > 256) {
    set_error("k_score_prior_rows: num_classes %d out of range", num_classes);
    return DDP_E_BADCFG;
  }
  const int chunks = (num_classes + 63) / 64, tiles_n = (N + SP_TILE - 1) / SP_TILE;
  const size_t blocks = size_t(B) * tiles_n * chunks;
  if (blocks > 0x7fffffffu) {
    set_error("k_score_prior_rows: %zu blocks", blocks);
    return DDP_E_BADCFG;
  }
  hipLaunchKernelGGL(k_score_prior_rows, dim3(unsigned(blocks)), dim3(256), 0, st, map, rows, num_classes, N, tiles_n, chunks);
  return check_launch("k_score_prior_rows");
}

}  // namespace ddp
