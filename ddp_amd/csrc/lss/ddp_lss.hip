// libddp_lss.so (include/ddp_lss_mi355x.h): the lift and pool of the reference's LSSTransform without the (B, N, D, fH, fW, C) volume.
// An integer plan (rank table, per-cell ascending point lists) and a floating-point pool over it.  DESIGN.md §8.3 has the design.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../../include/ddp_lss_mi355x.h"

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
  if (e == hipSuccess) return DDP_LSS_OK;
  return fail(DDP_LSS_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int SCAN_THREADS = 1024;
constexpr int SCAN_TILE = THREADS * 4;  // counts a block of the tiled scan owns
constexpr int LSS_RUN = 32;   // consecutive iy cells of one (b, z, ix) a pooling block owns: 128 B of every channel plane
constexpr int PRE_PIX = 64;   // pixels of one camera a pre-pass block owns
constexpr int PRE_CH = 64;    // channels transposed per LDS tile: 256-B segments of the context rows

// ---- derived sizes and the workspace ---------------------------------------------------------------------------------------------
struct Dims {
  int P, K, X;       // points, cells, pixels
  int HW, DHW, NDHW; // per camera plane, per camera, per sample
};

struct Carve {
  int* ranks;
  int* offs;
  int* cursor;
  int* sums;
  int* tmp;
  int* list;
  float* prob;
  float* rows;
  size_t bytes;
};

size_t round_up(size_t n) { return (n + (DDP_LSS_WS_ALIGN - 1)) / DDP_LSS_WS_ALIGN * DDP_LSS_WS_ALIGN; }

Carve carve(const Dims& d, int C, void* ws) {
  char* p = static_cast<char*>(ws);
  size_t o = 0;
  Carve c;
  auto take = [&](size_t n) { char* q = p + o; o += round_up(n); return q; };
  c.ranks = reinterpret_cast<int*>(take(4 * (size_t)d.P));
  c.offs = reinterpret_cast<int*>(take(4 * ((size_t)d.K + 1)));
  c.cursor = reinterpret_cast<int*>(take(4 * (size_t)d.K));
  c.sums = reinterpret_cast<int*>(take(4 * (((size_t)d.K + SCAN_TILE - 1) / SCAN_TILE)));
  c.tmp = reinterpret_cast<int*>(take(4 * (size_t)d.P));
  c.list = reinterpret_cast<int*>(take(4 * (size_t)d.P));
  c.prob = reinterpret_cast<float*>(take(4 * (size_t)d.P));
  c.rows = reinterpret_cast<float*>(take(4 * (size_t)d.X * C));
  c.bytes = o;
  return c;
}

bool mul_lt_2_31(long long& acc, int f) {
  acc *= f;  // acc < 2^31 and f < 2^31 on entry: no overflow of the 64-bit product
  return acc < (1ll << 31);
}

int check_cfg(const ddp_lss_cfg* cfg, Dims* out) {
  if (!cfg) return fail(DDP_LSS_E_NULL, "cfg is NULL");
  if (cfg->channels < 1 || cfg->channels > DDP_LSS_MAX_CHANNELS)
    return fail(DDP_LSS_E_BADCFG, "channels %d out of range [1,%d]", cfg->channels, DDP_LSS_MAX_CHANNELS);
  if (cfg->depth_bins < 1 || cfg->depth_bins > DDP_LSS_MAX_DEPTH_BINS)
    return fail(DDP_LSS_E_BADCFG, "depth_bins %d out of range [1,%d]", cfg->depth_bins, DDP_LSS_MAX_DEPTH_BINS);
  const int ext[] = {cfg->batch, cfg->cams, cfg->feat_h, cfg->feat_w, cfg->image_h, cfg->image_w, cfg->nx[0], cfg->nx[1], cfg->nx[2]};
  const char* names[] = {"batch", "cams", "feat_h", "feat_w", "image_h", "image_w", "nx[0]", "nx[1]", "nx[2]"};
  for (int i = 0; i < 9; ++i)
    if (ext[i] < 1) return fail(DDP_LSS_E_BADCFG, "extent %s = %d must be positive", names[i], ext[i]);
  const double* bounds[] = {cfg->dbound, cfg->xbound, cfg->ybound, cfg->zbound};
  const char* bnames[] = {"dbound", "xbound", "ybound", "zbound"};
  for (int i = 0; i < 4; ++i) {
    if (!std::isfinite(bounds[i][0]) || !std::isfinite(bounds[i][1]) || !std::isfinite(bounds[i][2]) || !(bounds[i][2] > 0.0))
      return fail(DDP_LSS_E_BADCFG, "%s must be finite with a positive step", bnames[i]);
  }
  long long P = cfg->batch, K = cfg->batch;
  if (!mul_lt_2_31(P, cfg->cams) || !mul_lt_2_31(P, cfg->depth_bins) || !mul_lt_2_31(P, cfg->feat_h) || !mul_lt_2_31(P, cfg->feat_w))
    return fail(DDP_LSS_E_BADCFG, "too many points: B*N*D*fH*fW must stay below 2^31");
  if (!mul_lt_2_31(K, cfg->nx[2]) || !mul_lt_2_31(K, cfg->nx[0]) || !mul_lt_2_31(K, cfg->nx[1]))
    return fail(DDP_LSS_E_BADCFG, "too many cells: B*nz*nx0*nx1 must stay below 2^31");
  if (out) {
    out->P = int(P);
    out->K = int(K);
    out->HW = cfg->feat_h * cfg->feat_w;
    out->DHW = cfg->depth_bins * out->HW;
    out->NDHW = cfg->cams * out->DHW;
    out->X = cfg->batch * cfg->cams * out->HW;
  }
  return DDP_LSS_OK;
}

int check_ptr(const void* p, const char* name, unsigned align) {
  if (!p) return fail(DDP_LSS_E_NULL, "%s is NULL", name);
  if (reinterpret_cast<uintptr_t>(p) & (align - 1)) return fail(DDP_LSS_E_ALIGN, "%s must be %u-byte aligned", name, align);
  return DDP_LSS_OK;
}

// ---- plan: ranks ------------------------------------------------------------------------------------------------------------------
struct GeomArgs {
  int P, K, D, fH, fW, HW, DHW, NDHW, N;
  int nx0, nx1, nz;
  float x_end, x_step, y_end, y_step;  // linspace(0, end, steps): step = end / (steps - 1) in fp32
  double d_lo, d_step;                 // arange in double, rounded once
  float lo[3], dx[3];                  // bx - dx / 2 and dx per axis, fp32
};

// torch.linspace(0, end, steps, dtype=float)[i]; one step is the start alone
__device__ __forceinline__ float lss_linspace(float end, float step, int steps, int i) {
  if (steps == 1) return 0.f;
  return i < steps / 2 ? __fmul_rn(step, float(i)) : __fsub_rn(end, __fmul_rn(step, float(steps - i - 1)));
}

// row-major 3 x 3 times vector, one rounding per operation, summed left to right
__device__ __forceinline__ void lss_mat3(const float* __restrict__ m, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = __fadd_rn(__fadd_rn(__fmul_rn(m[0], x), __fmul_rn(m[1], y)), __fmul_rn(m[2], z));
  oy = __fadd_rn(__fadd_rn(__fmul_rn(m[3], x), __fmul_rn(m[4], y)), __fmul_rn(m[5], z));
  oz = __fadd_rn(__fadd_rn(__fmul_rn(m[6], x), __fmul_rn(m[7], y)), __fmul_rn(m[8], z));
}

// the cell along one axis, or -1: trunc((g - lo) / dx) toward zero, kept when 0 <= i < n.  NaN and +-inf fail the comparisons.
__device__ __forceinline__ int lss_cell(float g, float lo, float dx, int n) {
  const float q = __fdiv_rn(__fsub_rn(g, lo), dx);
  if (!(q > -1.0f && q < 2147483648.0f)) return -1;
  const int i = int(q);  // truncation: q in (-1, 0) gives 0
  return i < n ? i : -1;
}

__global__ void __launch_bounds__(THREADS) k_lss_rank(const GeomArgs a, const float* __restrict__ cam, const float* __restrict__ extra,
                                                       int* __restrict__ ranks, int* __restrict__ count) {
  const int p = blockIdx.x * THREADS + threadIdx.x;  // grid * THREADS < 2^31 + THREADS: P < 2^31 is checked by the host
  if (p >= a.P || p < 0) return;
  const int b = p / a.NDHW;
  const int bn = p / a.DHW;
  const int rem = p - bn * a.DHW;
  const int d = rem / a.HW;
  const int hw = rem - d * a.HW;
  const int h = hw / a.fW, w = hw - h * a.fW;
  const float* c = cam + (size_t)bn * 24;
  const float* e = extra + (size_t)b * 12;
  const float fx = lss_linspace(a.x_end, a.x_step, a.fW, w);
  const float fy = lss_linspace(a.y_end, a.y_step, a.fH, h);
  const float fd = float(a.d_lo + double(d) * a.d_step);
  float x = __fsub_rn(fx, c[9]), y = __fsub_rn(fy, c[10]), z = __fsub_rn(fd, c[11]);
  float u, v, t;
  lss_mat3(c, x, y, z, u, v, t);
  x = __fmul_rn(u, t); y = __fmul_rn(v, t); z = t;
  lss_mat3(c + 12, x, y, z, u, v, t);
  u = __fadd_rn(u, c[21]); v = __fadd_rn(v, c[22]); t = __fadd_rn(t, c[23]);
  lss_mat3(e, u, v, t, x, y, z);
  x = __fadd_rn(x, e[9]); y = __fadd_rn(y, e[10]); z = __fadd_rn(z, e[11]);
  const int ix = lss_cell(x, a.lo[0], a.dx[0], a.nx0);
  const int iy = lss_cell(y, a.lo[1], a.dx[1], a.nx1);
  const int iz = lss_cell(z, a.lo[2], a.dx[2], a.nz);
  int r = -1;
  if (ix >= 0 && iy >= 0 && iz >= 0) r = ((b * a.nz + iz) * a.nx0 + ix) * a.nx1 + iy;  // < K < 2^31
  ranks[p] = r;
  if (r >= 0) atomicAdd(&count[r], 1);
}

__global__ void __launch_bounds__(THREADS) k_lss_take_ranks(int P, int K, const int* __restrict__ src, int* __restrict__ ranks,
                                                             int* __restrict__ count) {
  const int p = blockIdx.x * THREADS + threadIdx.x;
  if (p >= P || p < 0) return;
  int r = src[p];
  if (r < 0 || r >= K) r = -1;
  ranks[p] = r;
  if (r >= 0) atomicAdd(&count[r], 1);
}

// ---- plan: lists ------------------------------------------------------------------------------------------------------------------
// The exclusive scan of the K counts, in three launches: a block sums a tile of SCAN_TILE counts; one block scans the tile sums
// (few: K / SCAN_TILE); a block scans its tile again and adds the tile's start.  `cursor` holds the counts on entry and the
// segment starts on exit; `offs` gets the same starts and, at [K], the number of kept points.
__device__ __forceinline__ int4 lss_tile_counts(int K, const int* __restrict__ cursor, long long i0) {
  int4 c = make_int4(0, 0, 0, 0);  // i0 is a multiple of 4 and the table is 256-byte aligned: one 16-byte load when all four exist
  if (i0 + 3 < K) return *reinterpret_cast<const int4*>(cursor + i0);
  if (i0 < K) c.x = cursor[i0];
  if (i0 + 1 < K) c.y = cursor[i0 + 1];
  if (i0 + 2 < K) c.z = cursor[i0 + 2];
  return c;
}

// inclusive scan of one value per thread over the block -> the thread's EXCLUSIVE prefix; *total = the block's sum
__device__ __forceinline__ int lss_block_excl(int v, int* wsum, int* total) {
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  int incl = v;
  for (int d = 1; d < WAVE; d <<= 1) {
    const int t = __shfl_up(incl, d, WAVE);
    if (lane >= d) incl += t;
  }
  if (lane == WAVE - 1) wsum[wave] = incl;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < WAVES; ++w) {
    if (w < wave) before += wsum[w];
    all += wsum[w];
  }
  *total = all;
  return before + incl - v;
}

__global__ void __launch_bounds__(THREADS) k_lss_tile_sums(int K, const int* __restrict__ cursor, int* __restrict__ sums) {
  __shared__ int wsum[WAVES];
  const int4 c = lss_tile_counts(K, cursor, (long long)blockIdx.x * SCAN_TILE + threadIdx.x * 4);
  int total;
  lss_block_excl(c.x + c.y + c.z + c.w, wsum, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: in-place exclusive scan of n values, *total = their sum
__global__ void __launch_bounds__(SCAN_THREADS) k_lss_scan(int n, int* __restrict__ v, int* __restrict__ total) {
  __shared__ int part[SCAN_THREADS];
  const int tid = threadIdx.x;
  const long long per = ((long long)n + SCAN_THREADS - 1) / SCAN_THREADS;
  const long long lo = tid * per < n ? tid * per : n;
  const long long hi = lo + per < n ? lo + per : n;
  int s = 0;
  for (long long i = lo; i < hi; ++i) s += v[i];
  part[tid] = s;
  __syncthreads();
  for (int d = 1; d < SCAN_THREADS; d <<= 1) {
    const int t = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += t;
    __syncthreads();
  }
  int run = part[tid] - s;
  for (long long i = lo; i < hi; ++i) {
    const int c = v[i];
    v[i] = run;
    run += c;
  }
  if (tid == SCAN_THREADS - 1) *total = part[tid];
}

__global__ void __launch_bounds__(THREADS) k_lss_tile_scan(int K, int* __restrict__ cursor, int* __restrict__ offs, const int* __restrict__ sums) {
  __shared__ int wsum[WAVES];
  const long long i0 = (long long)blockIdx.x * SCAN_TILE + threadIdx.x * 4;
  const int4 c = lss_tile_counts(K, cursor, i0);
  int total;
  const int s0 = sums[blockIdx.x] + lss_block_excl(c.x + c.y + c.z + c.w, wsum, &total);
  const int s1 = s0 + c.x, s2 = s1 + c.y, s3 = s2 + c.z;
  if (i0 + 3 < K) {
    *reinterpret_cast<int4*>(cursor + i0) = make_int4(s0, s1, s2, s3);
    *reinterpret_cast<int4*>(offs + i0) = make_int4(s0, s1, s2, s3);
  } else {
    if (i0 < K) cursor[i0] = offs[i0] = s0;
    if (i0 + 1 < K) cursor[i0 + 1] = offs[i0 + 1] = s1;
    if (i0 + 2 < K) cursor[i0 + 2] = offs[i0 + 2] = s2;
  }
}

// every kept point takes the next slot of its cell: the order inside a segment is that of the atomics, k_lss_sort removes it
__global__ void __launch_bounds__(THREADS) k_lss_fill(int P, const int* __restrict__ ranks, int* __restrict__ cursor, int* __restrict__ tmp) {
  const int p = blockIdx.x * THREADS + threadIdx.x;
  if (p >= P || p < 0) return;
  const int r = ranks[p];
  if (r < 0) return;
  const int slot = atomicAdd(&cursor[r], 1);  // < offs[r + 1] <= P: the counts were taken from the same table
  tmp[slot] = p;
}

// A wave per cell: entry e goes to position #{entries of the segment smaller than e}.  Point ids are distinct, so the positions are
// a permutation of the segment, and the sorted segment does not depend on the order k_lss_fill left.
__global__ void __launch_bounds__(THREADS) k_lss_sort(int K, const int* __restrict__ offs, const int* __restrict__ tmp, int* __restrict__ list) {
  const int lane = threadIdx.x % WAVE;
  const long long cell_ll = (long long)blockIdx.x * WAVES + threadIdx.x / WAVE;
  if (cell_ll >= K) return;
  const int cell = __builtin_amdgcn_readfirstlane(int(cell_ll));
  const int o0 = __builtin_amdgcn_readfirstlane(offs[cell]);
  const int L = __builtin_amdgcn_readfirstlane(offs[cell + 1]) - o0;
  for (int i0 = 0; i0 < L; i0 += WAVE) {
    const int i = i0 + lane;
    const int e = i < L ? tmp[o0 + i] : INT_MAX;
    int pos = 0;
    for (int j0 = 0; j0 < L; j0 += WAVE) {
      const int v = j0 + lane < L ? tmp[o0 + j0 + lane] : INT_MAX;
      // all 64 lanes of the chunk, with constant lane selects: a lane past the segment holds INT_MAX, which is below no entry
#pragma unroll
      for (int j = 0; j < WAVE; ++j) pos += __builtin_amdgcn_readlane(v, j) < e ? 1 : 0;
    }
    if (i < L) list[o0 + pos] = e;  // pos < L
  }
}

// ---- pool: pre-pass ---------------------------------------------------------------------------------------------------------------
// A block owns PRE_PIX pixels of one camera.  Thread (s, px): the depth bins s, s + 4, ... of pixel px.  Writes the softmax
// probability per point (the layout of the first D input channels) and the C context channels of every pixel as one row.
__global__ void __launch_bounds__(THREADS) k_lss_pre(int D, int C, int HW, int tiles, const float* __restrict__ x, float* __restrict__ prob,
                                                      float* __restrict__ rows) {
  __shared__ float red[WAVES][PRE_PIX];
  __shared__ float tile[PRE_PIX][PRE_CH + 1];
  const int lane = threadIdx.x % WAVE, s = threadIdx.x / WAVE;
  const int bn = blockIdx.x / tiles, t = blockIdx.x - bn * tiles;
  const int px = t * PRE_PIX + lane;
  const bool valid = px < HW;
  const float* in = x + (size_t)bn * (D + C) * HW;
  float m = -INFINITY;
  if (valid)
    for (int d = s; d < D; d += WAVES) m = fmaxf(m, in[(size_t)d * HW + px]);
  red[s][lane] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0][lane], red[1][lane]), fmaxf(red[2][lane], red[3][lane]));
  __syncthreads();
  float sum = 0.f;
  if (valid)
    for (int d = s; d < D; d += WAVES) sum += expf(in[(size_t)d * HW + px] - m);
  red[s][lane] = sum;
  __syncthreads();
  sum = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
  if (valid) {
    float* out = prob + (size_t)bn * D * HW;  // (bn * D + d) * HW + px = the point index
    for (int d = s; d < D; d += WAVES) out[(size_t)d * HW + px] = __fdiv_rn(expf(in[(size_t)d * HW + px] - m), sum);
  }
  for (int c0 = 0; c0 < C; c0 += PRE_CH) {
    __syncthreads();
    for (int c = s; c < PRE_CH && c0 + c < C; c += WAVES) tile[lane][c] = valid ? in[(size_t)(D + c0 + c) * HW + px] : 0.f;
    __syncthreads();
    for (int q = s; q < PRE_PIX; q += WAVES) {
      const int pq = t * PRE_PIX + q;
      if (pq < HW && c0 + lane < C) rows[((size_t)bn * HW + pq) * C + c0 + lane] = tile[q][lane];
    }
  }
}

// ---- pool -------------------------------------------------------------------------------------------------------------------------
struct PoolArgs {
  int C, HW, DHW, nx0, nx1, nz, runs;  // runs: blocks per row of nx1 cells
};

// A block owns LSS_RUN consecutive iy cells of one (b, z, ix); a wave owns every fourth of them.  The wave walks a cell's list in
// order, 64 entries at a time (each lane fetches one entry, its probability and its pixel; the walk broadcasts them), lane l sums
// channels l, l + 64, ...  The sums go to LDS as [C][run] and leave as whole runs per channel plane.
template <int NCH>
__global__ void __launch_bounds__(THREADS) k_lss_pool(const PoolArgs a, const int* __restrict__ offs, const int* __restrict__ list,
                                                       const float* __restrict__ prob, const float* __restrict__ rows, float* __restrict__ out) {
  extern __shared__ float stage[];  // [C][LSS_RUN + 1]
  const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  const int row = blockIdx.x / a.runs;  // over (b, z, ix)
  const int iy0 = (blockIdx.x - row * a.runs) * LSS_RUN;
  for (int r = wave; r < LSS_RUN; r += WAVES) {
    float acc[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) acc[k] = 0.f;
    if (iy0 + r < a.nx1) {
      const int cell = row * a.nx1 + iy0 + r;  // < K
      const int o0 = __builtin_amdgcn_readfirstlane(offs[cell]);
      const int o1 = __builtin_amdgcn_readfirstlane(offs[cell + 1]);
      for (int base = o0; base < o1; base += WAVE) {
        const int n = o1 - base < WAVE ? o1 - base : WAVE;
        int mypix = 0;
        float mypr = 0.f;
        if (lane < n) {
          const int p = list[base + lane];
          mypr = prob[p];
          const int bn = p / a.DHW;
          mypix = bn * a.HW + (p - bn * a.DHW) % a.HW;
        }
        // four rows in flight; the sums still take the entries one by one, in list order
        int j = 0;
        for (; j + 4 <= n; j += 4) {
          float pr[4], v[4][NCH];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int pix = __builtin_amdgcn_readlane(mypix, j + u);
            pr[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mypr), j + u));
            const float* rp = rows + (size_t)pix * a.C;
#pragma unroll
            for (int k = 0; k < NCH; ++k) v[u][k] = lane + k * WAVE < a.C ? rp[lane + k * WAVE] : 0.f;
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < NCH; ++k) acc[k] = fmaf(pr[u], v[u][k], acc[k]);
        }
        for (; j < n; ++j) {
          const int pix = __builtin_amdgcn_readlane(mypix, j);
          const float pr = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mypr), j));
          const float* rp = rows + (size_t)pix * a.C;
#pragma unroll
          for (int k = 0; k < NCH; ++k)
            if (lane + k * WAVE < a.C) acc[k] = fmaf(pr, rp[lane + k * WAVE], acc[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      const int c = lane + k * WAVE;
      if (c < a.C) stage[c * (LSS_RUN + 1) + r] = acc[k];
    }
  }
  __syncthreads();
  const int per_b = a.nz * a.nx0;
  const int b = row / per_b, zi = row - b * per_b;  // zi = z * nx0 + ix
  const int z = zi / a.nx0, ix = zi - z * a.nx0;
  for (int idx = threadIdx.x; idx < a.C * LSS_RUN; idx += THREADS) {
    const int c = idx / LSS_RUN, r = idx % LSS_RUN;
    if (iy0 + r < a.nx1)
      out[((((size_t)b * a.nz + z) * a.C + c) * a.nx0 + ix) * a.nx1 + iy0 + r] = stage[c * (LSS_RUN + 1) + r];
  }
}

unsigned blocks_for(int n) { return unsigned(((long long)n + THREADS - 1) / THREADS); }

// counts -> offsets -> unsorted lists -> lists; the counts were added by the kernel that wrote the rank table
int finish_plan(const Dims& d, const Carve& w, hipStream_t st) {
  const unsigned tiles = unsigned(((long long)d.K + SCAN_TILE - 1) / SCAN_TILE);
  hipLaunchKernelGGL(k_lss_tile_sums, dim3(tiles), dim3(THREADS), 0, st, d.K, w.cursor, w.sums);
  hipLaunchKernelGGL(k_lss_scan, dim3(1), dim3(SCAN_THREADS), 0, st, int(tiles), w.sums, w.offs + d.K);
  hipLaunchKernelGGL(k_lss_tile_scan, dim3(tiles), dim3(THREADS), 0, st, d.K, w.cursor, w.offs, w.sums);
  hipLaunchKernelGGL(k_lss_fill, dim3(blocks_for(d.P)), dim3(THREADS), 0, st, d.P, w.ranks, w.cursor, w.tmp);
  hipLaunchKernelGGL(k_lss_sort, dim3(unsigned(((long long)d.K + WAVES - 1) / WAVES)), dim3(THREADS), 0, st, d.K, w.offs, w.tmp, w.list);
  return check_hip(hipGetLastError(), "plan kernels");
}

}  // namespace

extern "C" {

const char* ddp_lss_last_error(void) { return g_err; }

int ddp_lss_abi_version(void) { return DDP_LSS_ABI_VERSION; }

int ddp_lss_workspace(const ddp_lss_cfg* cfg, size_t* bytes) {
  if (!bytes) return fail(DDP_LSS_E_NULL, "bytes is NULL");
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  *bytes = carve(d, cfg->channels, nullptr).bytes;
  return DDP_LSS_OK;
}

int ddp_lss_ranks(const ddp_lss_cfg* cfg, void* d_workspace, const int32_t** d_ranks) {
  if (!d_ranks) return fail(DDP_LSS_E_NULL, "d_ranks is NULL");
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_LSS_WS_ALIGN)) return rc;
  *d_ranks = carve(d, cfg->channels, d_workspace).ranks;
  return DDP_LSS_OK;
}

int ddp_lss_plan(const ddp_lss_cfg* cfg, const float* d_cam, const float* d_extra, void* d_workspace, void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_ptr(d_cam, "d_cam", 4)) return rc;
  if (int rc = check_ptr(d_extra, "d_extra", 4)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_LSS_WS_ALIGN)) return rc;
  const Carve w = carve(d, cfg->channels, d_workspace);
  GeomArgs a;
  memset(&a, 0, sizeof(a));
  a.P = d.P; a.K = d.K; a.D = cfg->depth_bins; a.fH = cfg->feat_h; a.fW = cfg->feat_w;
  a.HW = d.HW; a.DHW = d.DHW; a.NDHW = d.NDHW; a.N = cfg->cams;
  a.nx0 = cfg->nx[0]; a.nx1 = cfg->nx[1]; a.nz = cfg->nx[2];
  a.x_end = float(cfg->image_w - 1);
  a.y_end = float(cfg->image_h - 1);
  a.x_step = cfg->feat_w > 1 ? a.x_end / float(cfg->feat_w - 1) : 0.f;
  a.y_step = cfg->feat_h > 1 ? a.y_end / float(cfg->feat_h - 1) : 0.f;
  a.d_lo = cfg->dbound[0];
  a.d_step = cfg->dbound[2];
  const double* bounds[3] = {cfg->xbound, cfg->ybound, cfg->zbound};
  for (int i = 0; i < 3; ++i) {
    const float dx = float(bounds[i][2]);
    const float bx = float(bounds[i][0] + bounds[i][2] / 2.0);
    a.dx[i] = dx;
    a.lo[i] = bx - dx / 2.0f;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = check_hip(hipMemsetAsync(w.cursor, 0, 4 * (size_t)d.K, st), "memset of the counts")) return rc;
  hipLaunchKernelGGL(k_lss_rank, dim3(blocks_for(d.P)), dim3(THREADS), 0, st, a, d_cam, d_extra, w.ranks, w.cursor);
  return finish_plan(d, w, st);
}

int ddp_lss_plan_from_ranks(const ddp_lss_cfg* cfg, const int32_t* d_ranks, void* d_workspace, void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_ptr(d_ranks, "d_ranks", 4)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_LSS_WS_ALIGN)) return rc;
  const Carve w = carve(d, cfg->channels, d_workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = check_hip(hipMemsetAsync(w.cursor, 0, 4 * (size_t)d.K, st), "memset of the counts")) return rc;
  hipLaunchKernelGGL(k_lss_take_ranks, dim3(blocks_for(d.P)), dim3(THREADS), 0, st, d.P, d.K, d_ranks, w.ranks, w.cursor);
  return finish_plan(d, w, st);
}

int ddp_lss_pool(const ddp_lss_cfg* cfg, const float* d_depthnet_out, void* d_workspace, float* d_out, void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_ptr(d_depthnet_out, "d_depthnet_out", 4)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_LSS_WS_ALIGN)) return rc;
  if (int rc = check_ptr(d_out, "d_out", 4)) return rc;
  const Carve w = carve(d, cfg->channels, d_workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int C = cfg->channels;
  const int tiles = (d.HW + PRE_PIX - 1) / PRE_PIX;
  const long long pre_blocks = (long long)cfg->batch * cfg->cams * tiles;  // <= X < 2^31
  hipLaunchKernelGGL(k_lss_pre, dim3(unsigned(pre_blocks)), dim3(THREADS), 0, st, cfg->depth_bins, C, d.HW, tiles, d_depthnet_out, w.prob, w.rows);
  PoolArgs a;
  a.C = C; a.HW = d.HW; a.DHW = d.DHW;
  a.nx0 = cfg->nx[0]; a.nx1 = cfg->nx[1]; a.nz = cfg->nx[2];
  a.runs = (cfg->nx[1] + LSS_RUN - 1) / LSS_RUN;
  const long long blocks = (long long)(d.K / cfg->nx[1]) * a.runs;  // <= K < 2^31
  const size_t lds = sizeof(float) * (size_t)C * (LSS_RUN + 1);
  const dim3 grid{unsigned(blocks)}, block{THREADS};
  switch ((C + WAVE - 1) / WAVE) {
    case 1: hipLaunchKernelGGL(k_lss_pool<1>, grid, block, lds, st, a, w.offs, w.list, w.prob, w.rows, d_out); break;
    case 2: hipLaunchKernelGGL(k_lss_pool<2>, grid, block, lds, st, a, w.offs, w.list, w.prob, w.rows, d_out); break;
    case 3: hipLaunchKernelGGL(k_lss_pool<3>, grid, block, lds, st, a, w.offs, w.list, w.prob, w.rows, d_out); break;
    default: hipLaunchKernelGGL(k_lss_pool<4>, grid, block, lds, st, a, w.offs, w.list, w.prob, w.rows, d_out); break;
  }
  return check_hip(hipGetLastError(), "pool kernels");
}

}  // extern "C"
