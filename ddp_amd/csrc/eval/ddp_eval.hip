// libddp_eval.so (include/ddp_eval_mi355x.h): the pre_eval statistics of the reference's test protocol, reduced on the device.
// Three tasks, each one launch (depth: a fixed-order second pass) plus the memset of its counter block.  DESIGN.md "Device
// evaluation" has the design of the seg kernel and the measured numbers.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../../include/ddp_eval_mi355x.h"

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
  if (e == hipSuccess) return DDP_EVAL_OK;
  return fail(DDP_EVAL_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;

// ---------------------------------------------------------------------------------------------------------------- seg ----
// A block owns SEG_TILE consecutive bytes of one item's (16-byte aligned) index space; a thread owns SEG_ITERS vectors of 16
// pixels.  Three levels keep equal keys away from the atomics (a key = (pred, l') of a pixel; label maps are piecewise constant,
// so neighbours share it):
//   thread  the 16 pixels of a vector are run-length coded in registers: one flush per run, not per pixel;
//   wave    when all 64 lanes hold one and the same constant vector (1024 pixels of one key), nothing is flushed at all: the wave
//           carries (key, count) in a wave-uniform register pair across its vectors and flushes when the key changes;
//   block   every wave adds into its OWN (3, 256) histogram in LDS (ds_add_u32, no return value), so waves never contend; the four
//           are summed at the end and each non-zero bin costs the block one global integer atomic.
constexpr int SEG_VEC = 16;
constexpr int SEG_ITERS = 2;
constexpr int SEG_TILE = THREADS * SEG_VEC * SEG_ITERS;  // 8192 pixels per block
constexpr int BINS = DDP_EVAL_SEG_BINS;

struct SegArgs {
  ddp_eval_seg_item items[DDP_EVAL_MAX_ITEMS];
  uint32_t off[DDP_EVAL_MAX_ITEMS];             // d_pred & 15 when both maps share it (vector path), else 0xffffffff (bytewise)
  uint32_t tile_start[DDP_EVAL_MAX_ITEMS + 1];  // first block of item i; [n_items] = grid size
  int n_items, K, ignore_index, reduce_zero_label;
};

__device__ __forceinline__ uint32_t seg_label(uint32_t l, int rzl) {
  return rzl ? ((l == 0u || l == 255u) ? 255u : l - 1u) : l;
}

// one run of `n` pixels with prediction p and mapped label l into the wave's histogram
__device__ __forceinline__ void seg_flush(uint32_t* h, uint32_t p, uint32_t l, uint32_t n, int K, int ign) {
  if (n == 0u || int(l) == ign) return;
  if (int(p) < K) {
    atomicAdd(&h[BINS + p], n);
    if (p == l) atomicAdd(&h[p], n);
  }
  if (int(l) < K) atomicAdd(&h[2 * BINS + l], n);
}

__global__ void __launch_bounds__(THREADS) k_eval_seg(const SegArgs a, uint32_t* __restrict__ counts) {
  __shared__ uint32_t hist[WAVES][3 * BINS];
  const int tid = threadIdx.x;
  for (int i = tid; i < WAVES * 3 * BINS; i += THREADS) (&hist[0][0])[i] = 0u;
  __syncthreads();

  // which item this block belongs to (block-uniform binary search in the kernel arguments)
  const uint32_t blk = blockIdx.x;
  int lo = 0, hi = a.n_items;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.tile_start[mid] <= blk) lo = mid; else hi = mid;
  }
  const int item = lo;
  const ddp_eval_seg_item it = a.items[item];
  const int K = a.K, ign = a.ignore_index, rzl = a.reduce_zero_label;
  const long long n = (long long)it.h * it.w;
  const uint32_t offv = a.off[item];
  const bool vec_ok = offv != 0xffffffffu;
  const long long off = vec_ok ? offv : 0;
  // the item's index space starts `off` bytes before its first pixel, where both maps are 16-byte aligned: pixel j sits at s = off + j
  const uint8_t* pp = it.d_pred - off;
  const uint8_t* lp = it.d_label - off;
  const long long s_begin = off, s_end = off + n;
  const long long tile0 = (long long)(blk - a.tile_start[item]) * SEG_TILE;

  uint32_t* h = hist[tid / WAVE];
  uint32_t wkey = 0u, wcnt = 0u;  // wave-uniform: the run the whole wave is in (key = p | l' << 8)

  for (int itv = 0; itv < SEG_ITERS; ++itv) {
    const long long s0 = tile0 + ((long long)itv * THREADS + tid) * SEG_VEC;
    const bool full = vec_ok && s0 >= s_begin && s0 + SEG_VEC <= s_end;
    bool uni = false;
    uint32_t key = 0u;
    uint4 pv = make_uint4(0, 0, 0, 0), lv = make_uint4(0, 0, 0, 0);
    if (full) {
      pv = *reinterpret_cast<const uint4*>(pp + s0);
      lv = *reinterpret_cast<const uint4*>(lp + s0);
      const uint32_t p0 = pv.x & 255u, l0 = lv.x & 255u;
      const uint32_t pb = p0 * 0x01010101u, lb = l0 * 0x01010101u;
      uni = ((pv.x ^ pb) | (pv.y ^ pb) | (pv.z ^ pb) | (pv.w ^ pb) | (lv.x ^ lb) | (lv.y ^ lb) | (lv.z ^ lb) | (lv.w ^ lb)) == 0u;
      key = p0 | (seg_label(l0, rzl) << 8);
    }
    // every lane of the wave reaches this point (the loop has no early exit)
    const uint32_t key0 = __builtin_amdgcn_readfirstlane(key);
    if (__all(uni && key == key0)) {
      if (key0 == wkey) {
        wcnt += WAVE * SEG_VEC;
      } else {
        if (tid % WAVE == 0) seg_flush(h, wkey & 255u, wkey >> 8, wcnt, K, ign);
        wkey = key0;
        wcnt = WAVE * SEG_VEC;
      }
      continue;
    }
    if (full) {
      if (uni) {
        seg_flush(h, key & 255u, key >> 8, SEG_VEC, K, ign);
      } else {
        const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w}, lw[4] = {lv.x, lv.y, lv.z, lv.w};
        uint32_t rp = pw[0] & 255u, rl = seg_label(lw[0] & 255u, rzl), rn = 0u;
#pragma unroll
        for (int j = 0; j < SEG_VEC; ++j) {
          const uint32_t p = (pw[j >> 2] >> (8 * (j & 3))) & 255u;
          const uint32_t l = seg_label((lw[j >> 2] >> (8 * (j & 3))) & 255u, rzl);
          if (p == rp && l == rl) {
            ++rn;
          } else {
            seg_flush(h, rp, rl, rn, K, ign);
            rp = p; rl = l; rn = 1u;
          }
        }
        seg_flush(h, rp, rl, rn, K, ign);
      }
    } else {
      // head, tail, or an item whose two maps disagree in alignment: byte loads, bounds checked per pixel
      const long long b = s0 > s_begin ? s0 : s_begin;
      const long long e = s0 + SEG_VEC < s_end ? s0 + SEG_VEC : s_end;
      uint32_t rp = 0u, rl = 0u, rn = 0u;
      for (long long s = b; s < e; ++s) {
        const uint32_t p = pp[s], l = seg_label(lp[s], rzl);
        if (rn != 0u && p == rp && l == rl) {
          ++rn;
        } else {
          seg_flush(h, rp, rl, rn, K, ign);
          rp = p; rl = l; rn = 1u;
        }
      }
      seg_flush(h, rp, rl, rn, K, ign);
    }
  }
  if (tid % WAVE == 0) seg_flush(h, wkey & 255u, wkey >> 8, wcnt, K, ign);
  __syncthreads();

  uint32_t* out = counts + (size_t)item * 3 * BINS;
  for (int i = tid; i < 3 * BINS; i += THREADS) {
    uint32_t v = 0u;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) v += hist[w][i];
    if (v != 0u) atomicAdd(&out[i], v);
  }
}

// -------------------------------------------------------------------------------------------------------------- depth ----
// pass 1: a block owns DEPTH_TILE consecutive pixels of one item's full map, a thread every THREADS-th of them; per-thread
// fp64 sums -> wave shuffle tree -> the four waves in order -> one row of DEPTH_NSUM doubles per block in the workspace.
// pass 2: one block per item adds that item's rows: thread t rows t, t + 256, ... in order, then the same tree.  Every order is
// fixed by the item's size alone, so a row of d_sums is the same bits wherever the item stands in a call.
constexpr int DEPTH_PER_THREAD = 4;                     // (fp64 logarithms: the pass is arithmetic bound, so many small blocks)
constexpr int DEPTH_TILE = THREADS * DEPTH_PER_THREAD;  // 1024 pixels per block
constexpr int DEPTH_NSUM = 10;

struct DepthArgs {
  ddp_eval_depth_item items[DDP_EVAL_MAX_ITEMS];
  uint32_t tile_start[DDP_EVAL_MAX_ITEMS + 1];
  int n_items;
  float min_depth, max_depth;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, WAVE);
  return v;  // lane 0
}

// sums[DEPTH_NSUM] of every thread -> out[DEPTH_NSUM] (written by thread 0), fixed order
__device__ __forceinline__ void block_sum(const double (&sums)[DEPTH_NSUM], double* out, double (*sh)[DEPTH_NSUM]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < DEPTH_NSUM; ++c) {
    const double v = wave_sum(sums[c]);
    if (tid % WAVE == 0) sh[tid / WAVE][c] = v;
  }
  __syncthreads();
  if (tid < DEPTH_NSUM) {
    double v = sh[0][tid];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v += sh[w][tid];
    out[tid] = v;
  }
}

__global__ void __launch_bounds__(THREADS) k_eval_depth_partial(const DepthArgs a, double* __restrict__ partial) {
  __shared__ double sh[WAVES][DEPTH_NSUM];
  const uint32_t blk = blockIdx.x;
  int lo = 0, hi = a.n_items;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.tile_start[mid] <= blk) lo = mid; else hi = mid;
  }
  const ddp_eval_depth_item it = a.items[lo];
  const long long n = (long long)it.h * it.w;
  const long long base = (long long)(blk - a.tile_start[lo]) * DEPTH_TILE;
  const float lo_d = a.min_depth, hi_d = a.max_depth;
  double s[DEPTH_NSUM];
#pragma unroll
  for (int c = 0; c < DEPTH_NSUM; ++c) s[c] = 0.0;
  for (int j = 0; j < DEPTH_PER_THREAD; ++j) {
    const long long i = base + (long long)j * THREADS + threadIdx.x;
    if (i >= n) break;
    const int y = int(i / it.w), x = int(i - (long long)y * it.w);
    if (y < it.y0 || y >= it.y1 || x < it.x0 || x >= it.x1) continue;
    const float g = it.d_gt[i];
    if (!(g > lo_d && g < hi_d)) continue;
    const float p = it.d_pred[i];
    const double gd = g, pd = p;
    // fp32 quotients, correctly rounded: the fp64 quotient of two fp32 values rounds to fp32 without a double-rounding error
    // (53 >= 2 * 24 + 2), and it is immune to the fp32 denormal mode of the kernel
    const float r0 = float(gd / pd), r1 = float(pd / gd);
    const float t = (r0 > r1 || r0 != r0) ? r0 : r1;  // np.maximum: NaN propagates
    s[0] += 1.0;
    s[1] += t < 1.25f ? 1.0 : 0.0;
    s[2] += t < 1.5625f ? 1.0 : 0.0;
    s[3] += t < 1.953125f ? 1.0 : 0.0;
    const double d = gd - pd, lg = log(gd), lpd = log(pd);
    s[4] += fabs(d) / gd;
    s[5] += d * d;
    s[6] += fabs(lg - lpd) * 0.43429448190325182765;  // |log10 g - log10 p| = |ln g - ln p| / ln 10: two logarithms fewer, one rounding more
    s[7] += (lg - lpd) * (lg - lpd);
    s[8] += lpd - lg;
    s[9] += d * d / gd;
  }
  block_sum(s, partial + (size_t)blk * DEPTH_NSUM, sh);
}

__global__ void __launch_bounds__(THREADS) k_eval_depth_final(const DepthArgs a, const double* __restrict__ partial,
                                                              double* __restrict__ sums) {
  __shared__ double sh[WAVES][DEPTH_NSUM];
  const int item = blockIdx.x;
  const uint32_t b0 = a.tile_start[item], b1 = a.tile_start[item + 1];
  double s[DEPTH_NSUM];
#pragma unroll
  for (int c = 0; c < DEPTH_NSUM; ++c) s[c] = 0.0;
  for (uint32_t b = b0 + threadIdx.x; b < b1; b += THREADS) {
#pragma unroll
    for (int c = 0; c < DEPTH_NSUM; ++c) s[c] += partial[(size_t)b * DEPTH_NSUM + c];
  }
  double* out = sums + (size_t)item * DDP_EVAL_DEPTH_COLS;
  block_sum(s, out, sh);
  if (threadIdx.x >= DEPTH_NSUM && threadIdx.x < DDP_EVAL_DEPTH_COLS) out[threadIdx.x] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------- bev ----
// grid (pixel tiles, classes, items).  Per thread and threshold: #hit and #(hit & label), plus #label once; tp = #(hit & label),
// fp = #hit - tp, fn = #label - tp.  Wave shuffle sums, the four waves through LDS, then one global integer atomic per non-zero
// counter and block.
constexpr int BEV_PER_THREAD = 8;
constexpr int BEV_TILE = THREADS * BEV_PER_THREAD;  // 2048 pixels per block
constexpr int MAXT = DDP_EVAL_MAX_THRESHOLDS;

struct BevArgs {
  ddp_eval_bev_item items[DDP_EVAL_MAX_ITEMS];
  float thr[MAXT];
  int K, n_pix, n_thr;
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int d = WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, WAVE);
  return v;
}

__global__ void __launch_bounds__(THREADS) k_eval_bev(const BevArgs a, uint32_t* __restrict__ counts) {
  const int k = blockIdx.y, item = blockIdx.z;
  const ddp_eval_bev_item it = a.items[item];
  const float* prob = it.d_prob + (size_t)k * a.n_pix;
  const uint8_t* gt = it.d_gt + (size_t)k * a.n_pix;
  uint32_t hit[MAXT], both[MAXT], lab = 0u;
#pragma unroll
  for (int t = 0; t < MAXT; ++t) hit[t] = both[t] = 0u;
  const long long base = (long long)blockIdx.x * BEV_TILE;
  for (int j = 0; j < BEV_PER_THREAD; ++j) {
    const long long i = base + (long long)j * THREADS + threadIdx.x;
    if (i >= a.n_pix) break;
    const float p = prob[i];
    const uint32_t l = gt[i] != 0 ? 1u : 0u;
    lab += l;
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      const uint32_t hh = (t < a.n_thr && p >= a.thr[t]) ? 1u : 0u;
      hit[t] += hh;
      both[t] += hh & l;
    }
  }
  __shared__ uint32_t sh[WAVES][2 * MAXT + 1];
  const int wave = threadIdx.x / WAVE;
  const uint32_t wl = wave_sum_u32(lab);
  if (threadIdx.x % WAVE == 0) sh[wave][2 * MAXT] = wl;
#pragma unroll
  for (int t = 0; t < MAXT; ++t) {
    if (t < a.n_thr) {  // uniform
      const uint32_t wh = wave_sum_u32(hit[t]), wb = wave_sum_u32(both[t]);
      if (threadIdx.x % WAVE == 0) {
        sh[wave][t] = wh;
        sh[wave][MAXT + t] = wb;
      }
    }
  }
  __syncthreads();
  if (int(threadIdx.x) < a.n_thr) {
    const int t = threadIdx.x;
    uint32_t bh = 0u, bb = 0u, bl = 0u;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
      bh += sh[w][t];
      bb += sh[w][MAXT + t];
      bl += sh[w][2 * MAXT];
    }
    uint32_t* out = counts + (((size_t)item * a.K + k) * a.n_thr + t) * 3;
    if (bb) atomicAdd(&out[0], bb);
    if (bh - bb) atomicAdd(&out[1], bh - bb);
    if (bl - bb) atomicAdd(&out[2], bl - bb);
  }
}

int check_items(const void* items, int n_items) {
  if (!items) return fail(DDP_EVAL_E_NULL, "items is NULL");
  if (n_items < 1 || n_items > DDP_EVAL_MAX_ITEMS)
    return fail(DDP_EVAL_E_BADCFG, "n_items %d out of range [1,%d]", n_items, DDP_EVAL_MAX_ITEMS);
  return DDP_EVAL_OK;
}

// validates the depth items and fills tile_start; -> DDP_EVAL_OK or the code already recorded
int depth_plan(const ddp_eval_depth_item* items, int n_items, DepthArgs* a, bool need_ptrs) {
  if (int rc = check_items(items, n_items)) return rc;
  unsigned long long blocks = 0;
  for (int i = 0; i < n_items; ++i) {
    const ddp_eval_depth_item& it = items[i];
    if (need_ptrs && (!it.d_pred || !it.d_gt)) return fail(DDP_EVAL_E_NULL, "depth item %d: NULL map", i);
    if (need_ptrs && ((reinterpret_cast<uintptr_t>(it.d_pred) | reinterpret_cast<uintptr_t>(it.d_gt)) & 3u))
      return fail(DDP_EVAL_E_ALIGN, "depth item %d: maps must be 4-byte aligned", i);
    if (it.h < 1 || it.w < 1 || (long long)it.h * it.w >= (1ll << 31))
      return fail(DDP_EVAL_E_BADCFG, "depth item %d: size %d x %d (1 <= h*w < 2^31)", i, it.h, it.w);
    if (it.y0 < 0 || it.y1 > it.h || it.x0 < 0 || it.x1 > it.w || it.y0 > it.y1 || it.x0 > it.x1)
      return fail(DDP_EVAL_E_BADCFG, "depth item %d: rectangle [%d,%d) x [%d,%d) outside the %d x %d map", i, it.y0, it.y1, it.x0,
                  it.x1, it.h, it.w);
    a->items[i] = it;
    a->tile_start[i] = uint32_t(blocks);
    blocks += ((unsigned long long)it.h * it.w + DEPTH_TILE - 1) / DEPTH_TILE;
    if (blocks >= (1ull << 31)) return fail(DDP_EVAL_E_BADCFG, "depth call too large: more than 2^31 blocks");
  }
  a->tile_start[n_items] = uint32_t(blocks);
  a->n_items = n_items;
  return DDP_EVAL_OK;
}

}  // namespace

extern "C" {

const char* ddp_eval_last_error(void) { return g_err; }

int ddp_eval_abi_version(void) { return DDP_EVAL_ABI_VERSION; }

int ddp_eval_seg(const ddp_eval_seg_item* items, int n_items, int num_classes, int ignore_index, int reduce_zero_label,
                 uint32_t* d_counts, void* stream) {
  if (int rc = check_items(items, n_items)) return rc;
  if (!d_counts) return fail(DDP_EVAL_E_NULL, "d_counts is NULL");
  if (reinterpret_cast<uintptr_t>(d_counts) & 3u) return fail(DDP_EVAL_E_ALIGN, "d_counts must be 4-byte aligned");
  if (num_classes < 2 || num_classes > BINS)
    return fail(DDP_EVAL_E_BADCFG, "num_classes %d out of range [2,%d] (the reference defines no answer for one class)", num_classes, BINS);
  SegArgs a;
  memset(&a, 0, sizeof(a));
  unsigned long long blocks = 0;
  for (int i = 0; i < n_items; ++i) {
    const ddp_eval_seg_item& it = items[i];
    if (!it.d_pred || !it.d_label) return fail(DDP_EVAL_E_NULL, "seg item %d: NULL map", i);
    if (it.h < 1 || it.w < 1 || (long long)it.h * it.w >= (1ll << 31))
      return fail(DDP_EVAL_E_BADCFG, "seg item %d: size %d x %d (1 <= h*w < 2^31)", i, it.h, it.w);
    const uint32_t op = uint32_t(reinterpret_cast<uintptr_t>(it.d_pred) & 15u), ol = uint32_t(reinterpret_cast<uintptr_t>(it.d_label) & 15u);
    a.items[i] = it;
    a.off[i] = op == ol ? op : 0xffffffffu;
    a.tile_start[i] = uint32_t(blocks);
    blocks += ((op == ol ? op : 0u) + (unsigned long long)it.h * it.w + SEG_TILE - 1) / SEG_TILE;
    if (blocks >= (1ull << 31)) return fail(DDP_EVAL_E_BADCFG, "seg call too large: more than 2^31 blocks");
  }
  a.tile_start[n_items] = uint32_t(blocks);
  a.n_items = n_items;
  a.K = num_classes;
  a.ignore_index = ignore_index;
  a.reduce_zero_label = reduce_zero_label ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = check_hip(hipMemsetAsync(d_counts, 0, (size_t)n_items * 3 * BINS * sizeof(uint32_t), st), "memset of the seg counters")) return rc;
  hipLaunchKernelGGL(k_eval_seg, dim3(uint32_t(blocks)), dim3(THREADS), 0, st, a, d_counts);
  return check_hip(hipGetLastError(), "k_eval_seg");
}

int ddp_eval_depth_workspace(const ddp_eval_depth_item* items, int n_items, size_t* bytes) {
  if (!bytes) return fail(DDP_EVAL_E_NULL, "bytes is NULL");
  DepthArgs a;
  if (int rc = depth_plan(items, n_items, &a, false)) return rc;
  *bytes = (size_t)a.tile_start[n_items] * DEPTH_NSUM * sizeof(double);
  return DDP_EVAL_OK;
}

int ddp_eval_depth(const ddp_eval_depth_item* items, int n_items, float min_depth, float max_depth, double* d_sums,
                   void* d_workspace, void* stream) {
  DepthArgs a;
  memset(&a, 0, sizeof(a));
  if (int rc = depth_plan(items, n_items, &a, true)) return rc;
  if (!d_sums || !d_workspace) return fail(DDP_EVAL_E_NULL, "d_sums / d_workspace is NULL");
  if ((reinterpret_cast<uintptr_t>(d_sums) | reinterpret_cast<uintptr_t>(d_workspace)) & 7u)
    return fail(DDP_EVAL_E_ALIGN, "d_sums and d_workspace must be 8-byte aligned");
  a.min_depth = min_depth;
  a.max_depth = max_depth;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_eval_depth_partial, dim3(a.tile_start[n_items]), dim3(THREADS), 0, st, a, static_cast<double*>(d_workspace));
  if (int rc = check_hip(hipGetLastError(), "k_eval_depth_partial")) return rc;
  hipLaunchKernelGGL(k_eval_depth_final, dim3(n_items), dim3(THREADS), 0, st, a, static_cast<const double*>(d_workspace), d_sums);
  return check_hip(hipGetLastError(), "k_eval_depth_final");
}

int ddp_eval_bev(const ddp_eval_bev_item* items, int n_items, int num_classes, int n_pix, const float* thresholds, int n_thr,
                 uint32_t* d_counts, void* stream) {
  if (int rc = check_items(items, n_items)) return rc;
  if (!thresholds || !d_counts) return fail(DDP_EVAL_E_NULL, "thresholds / d_counts is NULL");
  if (reinterpret_cast<uintptr_t>(d_counts) & 3u) return fail(DDP_EVAL_E_ALIGN, "d_counts must be 4-byte aligned");
  if (num_classes < 1 || num_classes > 65535) return fail(DDP_EVAL_E_BADCFG, "num_classes %d out of range [1,65535]", num_classes);
  if (n_pix < 1) return fail(DDP_EVAL_E_BADCFG, "n_pix %d out of range [1,2^31)", n_pix);
  if (n_thr < 1 || n_thr > MAXT) return fail(DDP_EVAL_E_BADCFG, "n_thr %d out of range [1,%d]", n_thr, MAXT);
  BevArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < n_items; ++i) {
    if (!items[i].d_prob || !items[i].d_gt) return fail(DDP_EVAL_E_NULL, "bev item %d: NULL map", i);
    if (reinterpret_cast<uintptr_t>(items[i].d_prob) & 3u) return fail(DDP_EVAL_E_ALIGN, "bev item %d: d_prob must be 4-byte aligned", i);
    a.items[i] = items[i];
  }
  for (int t = 0; t < n_thr; ++t) a.thr[t] = thresholds[t];
  a.K = num_classes;
  a.n_pix = n_pix;
  a.n_thr = n_thr;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = check_hip(hipMemsetAsync(d_counts, 0, (size_t)n_items * num_classes * n_thr * 3 * sizeof(uint32_t), st), "memset of the bev counters")) return rc;
  hipLaunchKernelGGL(k_eval_bev, dim3((n_pix + BEV_TILE - 1) / BEV_TILE, num_classes, n_items), dim3(THREADS), 0, st, a, d_counts);
  return check_hip(hipGetLastError(), "k_eval_bev");
}

}  // extern "C"
