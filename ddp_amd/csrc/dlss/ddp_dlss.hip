// libddp_dlss.so (include/ddp_dlss_mi355x.h): the front of the reference's DepthLSSTransform - lidar points projected into every
// camera, a deterministic scatter into the depth image, and the first two dtransform stages in one kernel.  DESIGN.md §8.4 has the
// design.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../../include/ddp_dlss_mi355x.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_hip(hipError_t e, const char* what) {
  if (e == hipSuccess) return DDP_DLSS_OK;
  return fail(DDP_DLSS_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int MID = DDP_DLSS_STEM_MID;
constexpr int OUT = DDP_DLSS_STEM_OUT;
constexpr int TAPS = 25;
// the folded stem parameters: s1[8], t1[8], w2[tap][c][o] (the 32 outputs of one (tap, c) are 128 contiguous bytes), bias2[32]
constexpr int FOLD_S1 = 0, FOLD_T1 = MID, FOLD_W2 = 2 * MID, FOLD_B2 = 2 * MID + TAPS * MID * OUT;
static_assert(FOLD_B2 + OUT == DDP_DLSS_STEM_FOLDED, "folded parameter count");
// a stem block owns ST_H output rows (one per wave) of ST_W output columns (one per lane) of one camera
constexpr int ST_W = WAVE, ST_H = WAVES;
constexpr int PATCH_W = 4 * ST_W + 1, PATCH_H = 4 * ST_H + 1;  // the 5 x 5 stride-4 windows of the tile: 17 x 257 depths

// ---- derived sizes and the workspace ---------------------------------------------------------------------------------------------
struct Dims {
  int T, X, HW, BN;  // table entries, pixels, pixels per camera, cameras
};

struct Carve {
  int* pix;
  float* dep;
  int* winner;
  float* fold;
  size_t bytes;
};

size_t round_up(size_t n) { return (n + (DDP_DLSS_WS_ALIGN - 1)) / DDP_DLSS_WS_ALIGN * DDP_DLSS_WS_ALIGN; }

Carve carve(const Dims& d, void* ws) {
  char* p = static_cast<char*>(ws);
  size_t o = 0;
  Carve c;
  auto take = [&](size_t n) { char* q = p + o; o += round_up(n); return q; };
  c.pix = reinterpret_cast<int*>(take(4 * (size_t)d.T));
  c.dep = reinterpret_cast<float*>(take(4 * (size_t)d.T));
  c.winner = reinterpret_cast<int*>(take(4 * (size_t)d.X));
  c.fold = reinterpret_cast<float*>(take(4 * (size_t)DDP_DLSS_STEM_FOLDED));
  c.bytes = o;
  return c;
}

int check_cfg(const ddp_dlss_cfg* cfg, Dims* out) {
  if (!cfg) return fail(DDP_DLSS_E_NULL, "cfg is NULL");
  const int ext[] = {cfg->batch, cfg->cams, cfg->image_h, cfg->image_w};
  const char* names[] = {"batch", "cams", "image_h", "image_w"};
  for (int i = 0; i < 4; ++i)
    if (ext[i] < 1) return fail(DDP_DLSS_E_BADCFG, "extent %s = %d must be positive", names[i], ext[i]);
  if (cfg->pmax < 0) return fail(DDP_DLSS_E_BADCFG, "pmax = %d must be in [0, 2^31)", cfg->pmax);
  const long long lim = 1ll << 31;
  const long long HW = (long long)cfg->image_h * cfg->image_w;
  if (HW >= lim) return fail(DDP_DLSS_E_BADCFG, "image too large: iH*iW must stay below 2^31");
  const long long BN = (long long)cfg->batch * cfg->cams;
  if (BN >= lim || BN * HW >= lim) return fail(DDP_DLSS_E_BADCFG, "too many pixels: B*N*iH*iW must stay below 2^31");
  if (BN * cfg->pmax >= lim) return fail(DDP_DLSS_E_BADCFG, "too many table entries: B*N*pmax must stay below 2^31");
  if (out) {
    out->BN = int(BN);
    out->HW = int(HW);
    out->X = int(BN * HW);
    out->T = int(BN * cfg->pmax);
  }
  return DDP_DLSS_OK;
}

int check_ptr(const void* p, const char* name, unsigned align) {
  if (!p) return fail(DDP_DLSS_E_NULL, "%s is NULL", name);
  if (reinterpret_cast<uintptr_t>(p) & (align - 1)) return fail(DDP_DLSS_E_ALIGN, "%s must be %u-byte aligned", name, align);
  return DDP_DLSS_OK;
}

unsigned blocks_for(long long n) { return unsigned((n + THREADS - 1) / THREADS); }

// ---- project ----------------------------------------------------------------------------------------------------------------------
// row-major 3 x 3 times vector, one rounding per operation, summed left to right
__device__ __forceinline__ void dlss_mat3(const float* __restrict__ m, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = __fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z));
  oy = __fadd_rn(__fadd_rn(__fmul_rn(m[3], x), __fmul_rn(m[4], y)), __fmul_rn(m[5], z));
  oz = __fadd_rn(__fadd_rn(__fmul_rn(m[6], x), __fmul_rn(m[7], y)), __fmul_rn(m[8], z));
}

// One sample: thread t = n * pmax + p is point p in camera n.  `pix` and `dep` are the sample's (N, pmax) slices.
__global__ void __launch_bounds__(THREADS) k_dlss_project(int pmax, int cams, int count, int stride, int iH, int iW,
                                                           const float* __restrict__ points, const float* __restrict__ lidar,
                                                           const float* __restrict__ cam, int* __restrict__ pix, float* __restrict__ dep) {
  const long long t_ll = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (t_ll >= (long long)cams * pmax) return;  // cams * pmax < 2^31 is checked by the host
  const int t = int(t_ll);
  const int n = t / pmax, p = t - n * pmax;
  if (p >= count) {
    pix[t] = -1;
    dep[t] = 0.f;
    return;
  }
  const float* q = points + (size_t)p * stride;
  const float* c = cam + (size_t)n * 24;
  float x = __fsub_rn(q[0], lidar[9]), y = __fsub_rn(q[1], lidar[10]), z = __fsub_rn(q[2], lidar[11]);
  float u, v, w;
  dlss_mat3(lidar, x, y, z, u, v, w);
  dlss_mat3(c, u, v, w, x, y, z);
  x = __fadd_rn(x, c[9]); y = __fadd_rn(y, c[10]); z = __fadd_rn(z, c[11]);
  z = z < 1e-5f ? 1e-5f : (z > 1e5f ? 1e5f : z);  // torch.clamp: a NaN stays a NaN
  x = __fdiv_rn(x, z); y = __fdiv_rn(y, z);
  dlss_mat3(c + 12, x, y, z, u, v, w);
  const float col = __fadd_rn(u, c[21]), row = __fadd_rn(v, c[22]);
  // as floats: NaN and +-inf fail; -0.0 passes and truncates to 0
  const bool on = row >= 0.f && row < float(iH) && col >= 0.f && col < float(iW);
  pix[t] = on ? int(row) * iW + int(col) : -1;  // < iH * iW < 2^31
  dep[t] = z;
}

// ---- scatter ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(THREADS) k_dlss_clear(int X, int* __restrict__ winner) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i < X) winner[i] = -1;
}

// entry t = (bn * pmax + p): the maximum of the point indices is the same whatever order the atomics arrive in
__global__ void __launch_bounds__(THREADS) k_dlss_vote(int T, int pmax, int HW, const int* __restrict__ pix, int* __restrict__ winner) {
  const long long t_ll = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (t_ll >= T) return;
  const int t = int(t_ll);
  const int px = pix[t];
  if (px < 0 || px >= HW) return;
  const int bn = t / pmax;
  atomicMax(&winner[(size_t)bn * HW + px], t - bn * pmax);
}

__global__ void __launch_bounds__(THREADS) k_dlss_resolve(int X, int pmax, int HW, const int* __restrict__ winner,
                                                           const float* __restrict__ dep, float* __restrict__ image) {
  const long long i_ll = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i_ll >= X) return;
  const int i = int(i_ll);
  const int w = winner[i];  // -1 or a point index the vote wrote: < pmax
  image[i] = w >= 0 && w < pmax ? dep[(size_t)(i / HW) * pmax + w] : 0.f;
}

// ---- stem -------------------------------------------------------------------------------------------------------------------------
struct StemPtrs {
  const float *w1, *b1, *g1, *be1, *m1, *v1, *w2, *b2, *g2, *be2, *m2, *v2;
  float eps1, eps2;
};

// one block: eval-mode BatchNorm folded into both convolutions; thread i folds the entries i, i + 256, ... of the conv2 weights
__global__ void __launch_bounds__(THREADS) k_dlss_fold(const StemPtrs s, float* __restrict__ fold) {
  const int tid = threadIdx.x;
  if (tid < MID) {
    const float g = __fdiv_rn(s.g1[tid], __fsqrt_rn(__fadd_rn(s.v1[tid], s.eps1)));
    fold[FOLD_S1 + tid] = __fmul_rn(s.w1[tid], g);
    fold[FOLD_T1 + tid] = __fadd_rn(__fmul_rn(__fsub_rn(s.b1[tid], s.m1[tid]), g), s.be1[tid]);
  }
  if (tid < OUT) {
    const float g = __fdiv_rn(s.g2[tid], __fsqrt_rn(__fadd_rn(s.v2[tid], s.eps2)));
    fold[FOLD_B2 + tid] = __fadd_rn(__fmul_rn(__fsub_rn(s.b2[tid], s.m2[tid]), g), s.be2[tid]);
  }
  for (int i = tid; i < TAPS * MID * OUT; i += THREADS) {
    const int o = i % OUT, c = (i / OUT) % MID, tap = i / (OUT * MID);
    const float g = __fdiv_rn(s.g2[o], __fsqrt_rn(__fadd_rn(s.v2[o], s.eps2)));
    fold[FOLD_W2 + i] = __fmul_rn(s.w2[(o * MID + c) * TAPS + tap], g);
  }
}

// Wave w of the block owns output row ty * ST_H + w, lane l output column tx * ST_W + l: every channel plane is stored in runs of 64
// columns.  The depth patch of the tile's windows is staged in LDS; a stage-1 activation is recomputed per tap (8 fma + max) and
// feeds 256 fma; the folded conv2 weights are read with wave-uniform addresses (scalar loads), 32 outputs per (tap, channel).
__global__ void __launch_bounds__(THREADS) k_dlss_stem(int iH, int iW, int oH, int oW, int tiles_x, int tiles_y,
                                                        const float* __restrict__ image, const float* __restrict__ fold,
                                                        float* __restrict__ out) {
  __shared__ float patch[PATCH_H][PATCH_W];
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const int tx = blockIdx.x % tiles_x;
  const int rest = blockIdx.x / tiles_x;
  const int ty = rest % tiles_y, bn = rest / tiles_y;
  const int y0 = ty * ST_H * 4 - 2, x0 = tx * ST_W * 4 - 2;  // image coordinates of patch[0][0]
  const float* img = image + (size_t)bn * iH * iW;
  for (int idx = threadIdx.x; idx < PATCH_H * PATCH_W; idx += THREADS) {
    const int r = idx / PATCH_W, c = idx - r * PATCH_W;
    const int iy = y0 + r, ix = x0 + c;
    patch[r][c] = iy >= 0 && iy < iH && ix >= 0 && ix < iW ? img[(size_t)iy * iW + ix] : 0.f;
  }
  __syncthreads();
  float s1[MID], t1[MID];
#pragma unroll
  for (int c = 0; c < MID; ++c) {
    s1[c] = fold[FOLD_S1 + c];
    t1[c] = fold[FOLD_T1 + c];
  }
  float acc[OUT];
#pragma unroll
  for (int o = 0; o < OUT; ++o) acc[o] = 0.f;
  const int oy = ty * ST_H + wave, ox = tx * ST_W + lane;
#pragma unroll 1
  for (int ky = 0; ky < 5; ++ky) {
    const int iy = 4 * oy - 2 + ky;
#pragma unroll 1
    for (int kx = 0; kx < 5; ++kx) {
      const int ix = 4 * ox - 2 + kx;
      const bool in = iy >= 0 && iy < iH && ix >= 0 && ix < iW;  // the padding pads the stage-1 OUTPUT: such a tap adds 0
      const float d = patch[4 * wave + ky][4 * lane + kx];
      const float* w = fold + FOLD_W2 + (ky * 5 + kx) * (MID * OUT);
#pragma unroll
      for (int c = 0; c < MID; ++c) {
        const float a = in ? fmaxf(fmaf(s1[c], d, t1[c]), 0.f) : 0.f;
#pragma unroll
        for (int o = 0; o < OUT; ++o) acc[o] = fmaf(w[c * OUT + o], a, acc[o]);
      }
    }
  }
  if (oy < oH && ox < oW) {
    float* dst = out + ((size_t)bn * OUT * oH + oy) * oW + ox;
#pragma unroll
    for (int o = 0; o < OUT; ++o) dst[(size_t)o * oH * oW] = fmaxf(__fadd_rn(acc[o], fold[FOLD_B2 + o]), 0.f);
  }
}

int run_scatter(const ddp_dlss_cfg* cfg, const Dims& d, const int* pix, const float* dep, int* winner, float* image, hipStream_t st) {
  hipLaunchKernelGGL(k_dlss_clear, dim3(blocks_for(d.X)), dim3(THREADS), 0, st, d.X, winner);
  if (d.T > 0) hipLaunchKernelGGL(k_dlss_vote, dim3(blocks_for(d.T)), dim3(THREADS), 0, st, d.T, cfg->pmax, d.HW, pix, winner);
  hipLaunchKernelGGL(k_dlss_resolve, dim3(blocks_for(d.X)), dim3(THREADS), 0, st, d.X, cfg->pmax, d.HW, winner, dep, image);
  return check_hip(hipGetLastError(), "scatter kernels");
}

}  // namespace

extern "C" {

const char* ddp_dlss_last_error(void) { return g_err; }

int ddp_dlss_abi_version(void) { return DDP_DLSS_ABI_VERSION; }

int ddp_dlss_workspace(const ddp_dlss_cfg* cfg, size_t* bytes) {
  if (!bytes) return fail(DDP_DLSS_E_NULL, "bytes is NULL");
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  *bytes = carve(d, nullptr).bytes;
  return DDP_DLSS_OK;
}

int ddp_dlss_pixels(const ddp_dlss_cfg* cfg, void* d_workspace, const int32_t** d_pixels, const float** d_depths) {
  if (!d_pixels) return fail(DDP_DLSS_E_NULL, "d_pixels is NULL");
  if (!d_depths) return fail(DDP_DLSS_E_NULL, "d_depths is NULL");
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_DLSS_WS_ALIGN)) return rc;
  const Carve w = carve(d, d_workspace);
  *d_pixels = w.pix;
  *d_depths = w.dep;
  return DDP_DLSS_OK;
}

int ddp_dlss_project(const ddp_dlss_cfg* cfg, const float* const* h_points, const int32_t* h_counts, int32_t stride,
                     const float* d_lidar, const float* d_cam, void* d_workspace, void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (stride < 3) return fail(DDP_DLSS_E_BADCFG, "stride = %d floats per point row must be at least 3", stride);
  if (!h_points) return fail(DDP_DLSS_E_NULL, "h_points is NULL");
  if (!h_counts) return fail(DDP_DLSS_E_NULL, "h_counts is NULL");
  for (int b = 0; b < cfg->batch; ++b) {
    if (h_counts[b] < 0) return fail(DDP_DLSS_E_BADCFG, "count[%d] = %d must not be negative", b, h_counts[b]);
    if (h_counts[b] > cfg->pmax) return fail(DDP_DLSS_E_BADCFG, "count[%d] = %d exceeds pmax = %d", b, h_counts[b], cfg->pmax);
    if (h_counts[b] > 0)
      if (int rc = check_ptr(h_points[b], "h_points[b]", 4)) return rc;
  }
  if (int rc = check_ptr(d_lidar, "d_lidar", 4)) return rc;
  if (int rc = check_ptr(d_cam, "d_cam", 4)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_DLSS_WS_ALIGN)) return rc;
  if (cfg->pmax == 0) return DDP_DLSS_OK;  // no table entry to write
  const Carve w = carve(d, d_workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int N = cfg->cams;
  const long long per = (long long)N * cfg->pmax;
  for (int b = 0; b < cfg->batch; ++b)
    hipLaunchKernelGGL(k_dlss_project, dim3(blocks_for(per)), dim3(THREADS), 0, st, cfg->pmax, N, h_counts[b], stride, cfg->image_h,
                       cfg->image_w, h_points[b], d_lidar + (size_t)b * 12, d_cam + (size_t)b * N * 24, w.pix + (size_t)b * per,
                       w.dep + (size_t)b * per);
  return check_hip(hipGetLastError(), "project kernels");
}

int ddp_dlss_scatter(const ddp_dlss_cfg* cfg, void* d_workspace, float* d_image, void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_DLSS_WS_ALIGN)) return rc;
  if (int rc = check_ptr(d_image, "d_image", 4)) return rc;
  const Carve w = carve(d, d_workspace);
  return run_scatter(cfg, d, w.pix, w.dep, w.winner, d_image, static_cast<hipStream_t>(stream));
}

int ddp_dlss_scatter_from_tables(const ddp_dlss_cfg* cfg, const int32_t* d_pixels, const float* d_depths, void* d_workspace,
                                 float* d_image, void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (d.T > 0) {
    if (int rc = check_ptr(d_pixels, "d_pixels", 4)) return rc;
    if (int rc = check_ptr(d_depths, "d_depths", 4)) return rc;
  }
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_DLSS_WS_ALIGN)) return rc;
  if (int rc = check_ptr(d_image, "d_image", 4)) return rc;
  const Carve w = carve(d, d_workspace);
  return run_scatter(cfg, d, d_pixels, d_depths, w.winner, d_image, static_cast<hipStream_t>(stream));
}

int ddp_dlss_stem(const ddp_dlss_cfg* cfg, const float* d_image, const ddp_dlss_stem_params* params, void* d_workspace, float* d_out,
                  void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_ptr(d_image, "d_image", 4)) return rc;
  if (!params) return fail(DDP_DLSS_E_NULL, "params is NULL");
  const float* const ptrs[] = {params->d_conv1_weight, params->d_conv1_bias, params->d_bn1_weight, params->d_bn1_bias,
                               params->d_bn1_mean,     params->d_bn1_var,    params->d_conv2_weight, params->d_conv2_bias,
                               params->d_bn2_weight,   params->d_bn2_bias,   params->d_bn2_mean,   params->d_bn2_var};
  const char* names[] = {"d_conv1_weight", "d_conv1_bias", "d_bn1_weight", "d_bn1_bias", "d_bn1_mean", "d_bn1_var",
                         "d_conv2_weight", "d_conv2_bias", "d_bn2_weight", "d_bn2_bias", "d_bn2_mean", "d_bn2_var"};
  for (int i = 0; i < 12; ++i)
    if (int rc = check_ptr(ptrs[i], names[i], 4)) return rc;
  if (!(params->bn1_eps >= 0.0) || !(params->bn2_eps >= 0.0) || !std::isfinite(params->bn1_eps) || !std::isfinite(params->bn2_eps))
    return fail(DDP_DLSS_E_BADCFG, "the BatchNorm eps must be finite and not negative");
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_DLSS_WS_ALIGN)) return rc;
  if (int rc = check_ptr(d_out, "d_out", 4)) return rc;
  const Carve w = carve(d, d_workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  StemPtrs s{ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], ptrs[7], ptrs[8], ptrs[9], ptrs[10], ptrs[11],
             float(params->bn1_eps), float(params->bn2_eps)};
  hipLaunchKernelGGL(k_dlss_fold, dim3(1), dim3(THREADS), 0, st, s, w.fold);
  const int oH = (cfg->image_h - 1) / 4 + 1, oW = (cfg->image_w - 1) / 4 + 1;
  const int tiles_x = (oW + ST_W - 1) / ST_W, tiles_y = (oH + ST_H - 1) / ST_H;
  const long long blocks = (long long)d.BN * tiles_x * tiles_y;  // <= B*N*iH*iW < 2^31
  hipLaunchKernelGGL(k_dlss_stem, dim3(unsigned(blocks)), dim3(THREADS), 0, st, cfg->image_h, cfg->image_w, oH, oW, tiles_x, tiles_y,
                     d_image, w.fold, d_out);
  return check_hip(hipGetLastError(), "stem kernels");
}

}  // extern "C"
