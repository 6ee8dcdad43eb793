// ddp_noise.hip - DDP_FLAG_SEEDED_NOISE: the start noise and the ddpm step noise of a call, generated on the device (gfx950, wave64).
//
// Philox4x32-10 (Salmon et al., SC'11) keyed by (seed_lo, seed_hi) with the counter (e >> 2, image, stream, call): `e` is the flat
// index of the element inside its image's (r, Cm, h, w) block and output lane e & 3 of that counter is the element's value, so a
// value is a function of (seed, image, stream, call, e) and of nothing else - not of the batch size, the position in the batch,
// the layout it is written in or the grid that wrote it.  Normals: Box-Muller on exact uniforms, lanes (0, 1) from words (0, 1)
// and lanes (2, 3) from words (2, 3), with the accurate library logf / sincospif / sqrtf.  The key words are read from DEVICE
// memory (include/ddp_mi355x.h), so a captured graph replays with whatever key the caller wrote in front of the launch.
// Two writers with identical values: k_noise_fill_nchw (NCHW, what every consumer of the caller's d_noise reads) and
// k_noise_fill_tok (token-major rows of 256 channels, what k_seg_update adds after a ddpm step).  Both are byte-streaming: no
// LDS, no scratch.
#include <math.h>
#include <stdint.h>
#include "ddp_internal.h"

namespace ddp {
namespace {

struct Normal4 {
  float v[4];
};

__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
  const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
  const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
  c[0] = n0;
  c[1] = lo1;
  c[2] = n2;
  c[3] = lo0;
}

// u = ((x >> 9) + 0.5) * 2^-23: 23 random bits and a half, exact in fp32, strictly inside (0, 1); 2 u is exact as well
__device__ __forceinline__ float uniform23(uint32_t x) { return (float(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// the four normals of counter (g, image, stream, call) under key (k0, k1)
__device__ __forceinline__ Normal4 philox_normal4(uint32_t g, uint32_t image, uint32_t stream, uint32_t call, uint32_t k0, uint32_t k1) {
  uint32_t c[4] = {g, image, stream, call};
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  Normal4 z;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float rad = sqrtf(-2.0f * logf(uniform23(c[2 * p])));
    float sn, cs;
    sincospif(2.0f * uniform23(c[2 * p + 1]), &sn, &cs);
    z.v[2 * p] = rad * cs;
    z.v[2 * p + 1] = rad * sn;
  }
  return z;
}

// key (8 words, device): {seed_lo, seed_hi, image_base, stream_base, call, 0, 0, 0}

// Start noise (stream = stream_base), NCHW: out[b * per + e], one thread per counter = 4 consecutive elements of one image; `groups`
// = ceil(per / 4), the last counter of an image is used in part when per % 4 != 0 (per-element stores then: rows of the next image
// are not 16-byte aligned)
__global__ void __launch_bounds__(256) k_noise_fill_nchw(const uint32_t* __restrict__ key, float* __restrict__ out, unsigned per,
                                                         unsigned groups, unsigned total) {
  const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const unsigned b = t / groups, g = t - b * groups;
  const Normal4 z = philox_normal4(g, key[2] + b, key[3], key[4], key[0], key[1]);
  float* o = out + size_t(b) * per + size_t(g) * 4;
  if ((per & 3u) == 0) {
    *reinterpret_cast<float4*>(o) = make_float4(z.v[0], z.v[1], z.v[2], z.v[3]);
  } else {
    const unsigned left = per - g * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (unsigned(i) < left) o[i] = z.v[i];
  }
}

// Noise added after step s (stream = stream_base + 1 + s), written token-major: out[(map * N + n) * 256 + c] holds element
// e = (ri * 256 + c) * N + n of image b, map = b * r + ri.  Thread c of block (map, j) takes the j-th counter that touches channel
// plane p = ri * 256 + c, i.e. four consecutive pixels of that plane, and stores them to four rows at column c: the 64 lanes of a
// wave write 64 consecutive channels, whole 256-byte lines.  With N % 4 != 0 a counter can straddle two planes (or two rows of the
// map): every element is placed on its own, and such a counter is evaluated by both planes' threads - no padding anywhere.
__global__ void __launch_bounds__(256) k_noise_fill_tok(const uint32_t* __restrict__ key, float* __restrict__ out, unsigned N,
                                                        unsigned r, unsigned gn, unsigned step) {
  const unsigned map = blockIdx.x / gn, j = blockIdx.x - map * gn;
  const unsigned b = map / r, ri = map - b * r, c = threadIdx.x;
  const unsigned first = (ri * 256u + c) * N, last = first + N - 1;      // (r * 256 * N < 2^32: validate()'s token limit)
  const unsigned g = (first >> 2) + j;
  if (g > (last >> 2)) return;
  const Normal4 z = philox_normal4(g, key[2] + b, key[3] + 1u + step, key[4], key[0], key[1]);
  float* o = out + size_t(map) * N * 256 + c;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned e = g * 4 + i;
    if (e >= first && e <= last) o[size_t(e - first) * 256] = z.v[i];
  }
}

}  // namespace

int launch_noise_fill_nchw(const uint32_t* key, float* out, int B, size_t per_image, hipStream_t st) {
  if (B <= 0 || per_image == 0) return DDP_OK;
  const size_t groups = (per_image + 3) / 4, total = groups * size_t(B);
  if (per_image >> 32 || total >> 31) {
    set_error("k_noise_fill_nchw: %zu elements per image x %d images is out of range", per_image, B);
    return DDP_E_BADCFG;
  }
  hipLaunchKernelGGL(k_noise_fill_nchw, dim3(unsigned((total + 255) / 256)), dim3(256), 0, st, key, out, unsigned(per_image),
                     unsigned(groups), unsigned(total));
  return check_launch("k_noise_fill_nchw");
}

int launch_noise_fill_tok(const uint32_t* key, float* out, int B, int r, int N, int step, hipStream_t st) {
  if (B <= 0 || r <= 0 || N <= 0) return DDP_OK;
  const size_t gn = (size_t(N) + 3) / 4 + 1, blocks = gn * size_t(B) * r;
  if ((size_t(r) * 256 * N) >> 32 || blocks >> 31) {
    set_error("k_noise_fill_tok: %d x %d maps of %d tokens are out of range", B, r, N);
    return DDP_E_BADCFG;
  }
  hipLaunchKernelGGL(k_noise_fill_tok, dim3(unsigned(blocks)), dim3(256), 0, st, key, out, unsigned(N), unsigned(r), unsigned(gn),
                     unsigned(step));
  return check_launch("k_noise_fill_tok");
}

}  // namespace ddp
