// libddp_cm.so (include/ddp_cm_mi355x.h): the K x K confusion matrix of the reference's tools/confusion_matrix.py, accumulated on
// the device.  One launch per call, plus the memsets of a zeroing call.  DESIGN.md §8.2 has the design and the measured numbers.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../../include/ddp_cm_mi355x.h"

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
  if (e == hipSuccess) return DDP_CM_OK;
  return fail(DDP_CM_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

constexpr int WAVE = 64;
constexpr int THREADS = 256;

// A block owns a tile of consecutive bytes of one item's (16-byte aligned) index space; a thread owns `iters` vectors of 16 pixels.
// The tile is CM_TILE pixels (iters = 2) while the call has at most CM_BLOCKS_FULL of them - one resident set of the chip at 8 blocks
// on each of 256 CUs; a larger call doubles the tile, up to 8 x, so that the blocks, and with them the flushes that meet on the ONE
// matrix of the call, stay near that number.
// The three levels of k_eval_seg (libddp_eval.so) keep equal keys away from the atomics, on the 16-bit key (l', pred):
//   thread  the 16 pixels of a vector are run-length coded in registers: one flush per run, not per pixel;
//   wave    when all 64 lanes hold one and the same constant vector, nothing is flushed: the wave carries (key, count) in a
//           wave-uniform register pair across its vectors and flushes when the key changes;
//   block   runs are added into ONE table of the block in LDS (16 KiB whatever K is, so the wave slots of a CU, not the LDS, bound
//           the blocks per CU); at the end each non-zero bin costs the block one global 64-bit integer atomic.
// K * K bins do not fit the LDS for every K (256 * 256 * 4 B = 256 KiB), so the table has two shapes, chosen by the host:
//   direct  K * K <= CM_WORDS: tab[l' * K + pred] is the count;
//   hashed  otherwise: CM_SLOTS open-addressed slots, tab[s] = bin + 1 (0 = empty), tab[CM_SLOTS + s] = count.  A slot is claimed by
//           a compare-and-swap on its tag; after CM_PROBES occupied slots the run goes to the matrix directly, as one global 64-bit
//           atomic - a full table costs time, never a count.
constexpr int CM_VEC = 16;
constexpr int CM_ITERS = 2;
constexpr int CM_TILE = THREADS * CM_VEC * CM_ITERS;  // 8192 pixels per block, times 1, 2, 4 or 8
constexpr int CM_MAX_SCALE = 8;
constexpr unsigned long long CM_BLOCKS_FULL = 2048;
constexpr int CM_WORDS = 4096;                        // 16 KiB of LDS
constexpr int CM_SLOTS = CM_WORDS / 2;
constexpr int CM_PROBES = 8;
constexpr int NTAL = DDP_CM_TALLY;

struct CmArgs {
  ddp_cm_item items[DDP_CM_MAX_ITEMS];
  uint32_t off[DDP_CM_MAX_ITEMS];             // d_pred & 15 when both maps share it (vector path), else 0xffffffff (bytewise)
  uint32_t tile_start[DDP_CM_MAX_ITEMS + 1];  // first block of item i; [n_items] = grid size
  int n_items, K, ignore_index, reduce_zero_label;
  int iters;                                  // vectors per thread: CM_ITERS * the tile scale
};

__device__ __forceinline__ uint32_t cm_label(uint32_t l, int rzl) {
  return rzl ? ((l == 0u || l == 255u) ? 255u : l - 1u) : l;
}

// one run of `n` pixels with prediction p and mapped label l into the block's table (tal: the block's tally, [1..3])
template <bool DIRECT>
__device__ __forceinline__ void cm_flush(uint32_t* tab, uint32_t* tal, unsigned long long* __restrict__ matrix, uint32_t p, uint32_t l,
                                         uint32_t n, int K, int ign) {
  if (n == 0u) return;
  if (int(l) == ign) { atomicAdd(&tal[1], n); return; }
  if (int(l) >= K) { atomicAdd(&tal[2], n); return; }
  if (int(p) >= K) { atomicAdd(&tal[3], n); return; }
  const uint32_t bin = l * uint32_t(K) + p;  // < K * K
  if (DIRECT) {
    atomicAdd(&tab[bin], n);
    return;
  }
  const uint32_t tag = bin + 1u;
  uint32_t s = (bin * 0x9E3779B1u) >> 21;  // 11 bits: < CM_SLOTS
  for (int i = 0; i < CM_PROBES; ++i) {
    uint32_t cur = __hip_atomic_load(&tab[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);  // a tag is written once and never changes
    if (cur == 0u) cur = atomicCAS(&tab[s], 0u, tag);
    if (cur == 0u || cur == tag) {
      atomicAdd(&tab[CM_SLOTS + s], n);
      return;
    }
    s = (s + 1u) & uint32_t(CM_SLOTS - 1);
  }
  atomicAdd(&matrix[bin], (unsigned long long)n);
}

template <bool DIRECT>
__global__ void __launch_bounds__(THREADS) k_cm_seg(const CmArgs a, unsigned long long* __restrict__ matrix,
                                                     unsigned long long* __restrict__ tally) {
  __shared__ uint4 tab4[CM_WORDS / 4];
  __shared__ uint32_t tal[NTAL];
  uint32_t* tab = reinterpret_cast<uint32_t*>(tab4);
  const int tid = threadIdx.x;
  const int K = a.K, ign = a.ignore_index, rzl = a.reduce_zero_label;
  const int used = DIRECT ? (K * K + 3) / 4 : CM_WORDS / 4;  // uint4 words of the table this launch touches
  for (int i = tid; i < used; i += THREADS) tab4[i] = make_uint4(0, 0, 0, 0);
  if (tid < NTAL) tal[tid] = 0u;
  __syncthreads();

  // which item this block belongs to (block-uniform binary search in the kernel arguments)
  const uint32_t blk = blockIdx.x;
  int lo = 0, hi = a.n_items;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.tile_start[mid] <= blk) lo = mid; else hi = mid;
  }
  const int item = lo;
  const ddp_cm_item it = a.items[item];
  const long long n = (long long)it.h * it.w;
  const uint32_t offv = a.off[item];
  const bool vec_ok = offv != 0xffffffffu;
  const long long off = vec_ok ? offv : 0;
  // the item's index space starts `off` bytes before its first pixel, where both maps are 16-byte aligned: pixel j sits at s = off + j
  const uint8_t* pp = it.d_pred - off;
  const uint8_t* lp = it.d_label - off;
  const long long s_begin = off, s_end = off + n;
  const int iters = a.iters;
  const long long tile = (long long)iters * (THREADS * CM_VEC);
  const long long tile0 = (long long)(blk - a.tile_start[item]) * tile;
  if (tid == 0) {  // the pixels of this tile
    const long long b = tile0 > s_begin ? tile0 : s_begin;
    const long long e = tile0 + tile < s_end ? tile0 + tile : s_end;
    if (e > b) atomicAdd(&tal[0], uint32_t(e - b));
  }

  uint32_t wkey = 0u, wcnt = 0u;  // wave-uniform: the run the whole wave is in (key = p | l' << 8)

  for (int itv = 0; itv < iters; ++itv) {
    const long long s0 = tile0 + ((long long)itv * THREADS + tid) * CM_VEC;
    const bool full = vec_ok && s0 >= s_begin && s0 + CM_VEC <= s_end;
    bool uni = false;
    uint32_t key = 0u;
    uint4 pv = make_uint4(0, 0, 0, 0), lv = make_uint4(0, 0, 0, 0);
    if (full) {
      pv = *reinterpret_cast<const uint4*>(pp + s0);
      lv = *reinterpret_cast<const uint4*>(lp + s0);
      const uint32_t p0 = pv.x & 255u, l0 = lv.x & 255u;
      const uint32_t pb = p0 * 0x01010101u, lb = l0 * 0x01010101u;
      uni = ((pv.x ^ pb) | (pv.y ^ pb) | (pv.z ^ pb) | (pv.w ^ pb) | (lv.x ^ lb) | (lv.y ^ lb) | (lv.z ^ lb) | (lv.w ^ lb)) == 0u;
      key = p0 | (cm_label(l0, rzl) << 8);
    }
    // every lane of the wave reaches this point (the loop has no early exit)
    const uint32_t key0 = __builtin_amdgcn_readfirstlane(key);
    if (__all(uni && key == key0)) {
      if (key0 == wkey) {
        wcnt += WAVE * CM_VEC;
      } else {
        if (tid % WAVE == 0) cm_flush<DIRECT>(tab, tal, matrix, wkey & 255u, wkey >> 8, wcnt, K, ign);
        wkey = key0;
        wcnt = WAVE * CM_VEC;
      }
      continue;
    }
    if (full) {
      if (uni) {
        cm_flush<DIRECT>(tab, tal, matrix, key & 255u, key >> 8, CM_VEC, K, ign);
      } else {
        const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w}, lw[4] = {lv.x, lv.y, lv.z, lv.w};
        uint32_t rp = pw[0] & 255u, rl = cm_label(lw[0] & 255u, rzl), rn = 0u;
#pragma unroll
        for (int j = 0; j < CM_VEC; ++j) {
          const uint32_t p = (pw[j >> 2] >> (8 * (j & 3))) & 255u;
          const uint32_t l = cm_label((lw[j >> 2] >> (8 * (j & 3))) & 255u, rzl);
          if (p == rp && l == rl) {
            ++rn;
          } else {
            cm_flush<DIRECT>(tab, tal, matrix, rp, rl, rn, K, ign);
            rp = p; rl = l; rn = 1u;
          }
        }
        cm_flush<DIRECT>(tab, tal, matrix, rp, rl, rn, K, ign);
      }
    } else {
      // head, tail, or an item whose two maps disagree in alignment: byte loads, bounds checked per pixel
      const long long b = s0 > s_begin ? s0 : s_begin;
      const long long e = s0 + CM_VEC < s_end ? s0 + CM_VEC : s_end;
      uint32_t rp = 0u, rl = 0u, rn = 0u;
      for (long long s = b; s < e; ++s) {
        const uint32_t p = pp[s], l = cm_label(lp[s], rzl);
        if (rn != 0u && p == rp && l == rl) {
          ++rn;
        } else {
          cm_flush<DIRECT>(tab, tal, matrix, rp, rl, rn, K, ign);
          rp = p; rl = l; rn = 1u;
        }
      }
      cm_flush<DIRECT>(tab, tal, matrix, rp, rl, rn, K, ign);
    }
  }
  if (tid % WAVE == 0) cm_flush<DIRECT>(tab, tal, matrix, wkey & 255u, wkey >> 8, wcnt, K, ign);
  __syncthreads();

  if (DIRECT) {
    for (int i = tid; i < K * K; i += THREADS) {
      const uint32_t v = tab[i];
      if (v != 0u) atomicAdd(&matrix[i], (unsigned long long)v);
    }
  } else {
    for (int i = tid; i < CM_SLOTS; i += THREADS) {
      const uint32_t tag = tab[i];
      if (tag != 0u) atomicAdd(&matrix[tag - 1u], (unsigned long long)tab[CM_SLOTS + i]);  // tag - 1 < K * K: written by cm_flush alone
    }
  }
  if (tally && tid < NTAL && tal[tid] != 0u) atomicAdd(&tally[tid], (unsigned long long)tal[tid]);
}

int check_classes(int num_classes) {
  if (num_classes < 2 || num_classes > 256)
    return fail(DDP_CM_E_BADCFG, "num_classes %d out of range [2,256]", num_classes);
  return DDP_CM_OK;
}

}  // namespace

extern "C" {

const char* ddp_cm_last_error(void) { return g_err; }

int ddp_cm_abi_version(void) { return DDP_CM_ABI_VERSION; }

int ddp_cm_workspace(int num_classes, size_t* bytes) {
  if (!bytes) return fail(DDP_CM_E_NULL, "bytes is NULL");
  if (int rc = check_classes(num_classes)) return rc;
  *bytes = 0;  // the block tables live in LDS
  return DDP_CM_OK;
}

int ddp_cm_seg(const ddp_cm_item* items, int n_items, int num_classes, int ignore_index, int reduce_zero_label, int accumulate,
               uint64_t* d_matrix, uint64_t* d_tally, void* d_workspace, void* stream) {
  (void)d_workspace;
  if (!items) return fail(DDP_CM_E_NULL, "items is NULL");
  if (n_items < 1 || n_items > DDP_CM_MAX_ITEMS)
    return fail(DDP_CM_E_BADCFG, "n_items %d out of range [1,%d]", n_items, DDP_CM_MAX_ITEMS);
  if (!d_matrix) return fail(DDP_CM_E_NULL, "d_matrix is NULL");
  if ((reinterpret_cast<uintptr_t>(d_matrix) | reinterpret_cast<uintptr_t>(d_tally)) & 7u)
    return fail(DDP_CM_E_ALIGN, "d_matrix and d_tally must be 8-byte aligned");
  if (int rc = check_classes(num_classes)) return rc;
  CmArgs a;
  memset(&a, 0, sizeof(a));
  unsigned long long span[DDP_CM_MAX_ITEMS], blocks = 0;  // span: an item's index space, head included
  for (int i = 0; i < n_items; ++i) {
    const ddp_cm_item& it = items[i];
    if (!it.d_pred || !it.d_label) return fail(DDP_CM_E_NULL, "cm item %d: NULL map", i);
    if (it.h < 1 || it.w < 1 || (long long)it.h * it.w >= (1ll << 31))
      return fail(DDP_CM_E_BADCFG, "cm item %d: size %d x %d (1 <= h*w < 2^31)", i, it.h, it.w);
    const uint32_t op = uint32_t(reinterpret_cast<uintptr_t>(it.d_pred) & 15u), ol = uint32_t(reinterpret_cast<uintptr_t>(it.d_label) & 15u);
    a.items[i] = it;
    a.off[i] = op == ol ? op : 0xffffffffu;
    span[i] = (op == ol ? op : 0u) + (unsigned long long)it.h * it.w;
    blocks += (span[i] + CM_TILE - 1) / CM_TILE;
  }
  int scale = 1;
  while (scale < CM_MAX_SCALE && blocks > CM_BLOCKS_FULL * scale) scale *= 2;
  const unsigned long long tile = (unsigned long long)CM_TILE * scale;
  blocks = 0;
  for (int i = 0; i < n_items; ++i) {
    a.tile_start[i] = uint32_t(blocks);
    blocks += (span[i] + tile - 1) / tile;
  }
  if (blocks >= (1ull << 31)) return fail(DDP_CM_E_BADCFG, "cm call too large: more than 2^31 blocks");
  a.iters = CM_ITERS * scale;
  a.tile_start[n_items] = uint32_t(blocks);
  a.n_items = n_items;
  a.K = num_classes;
  a.ignore_index = ignore_index;
  a.reduce_zero_label = reduce_zero_label ? 1 : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!accumulate) {
    if (int rc = check_hip(hipMemsetAsync(d_matrix, 0, (size_t)num_classes * num_classes * sizeof(uint64_t), st), "memset of the matrix")) return rc;
    if (d_tally)
      if (int rc = check_hip(hipMemsetAsync(d_tally, 0, DDP_CM_TALLY * sizeof(uint64_t), st), "memset of the tally")) return rc;
  }
  unsigned long long* m = reinterpret_cast<unsigned long long*>(d_matrix);
  unsigned long long* t = reinterpret_cast<unsigned long long*>(d_tally);
  if (num_classes * num_classes <= CM_WORDS)
    hipLaunchKernelGGL(k_cm_seg<true>, dim3(uint32_t(blocks)), dim3(THREADS), 0, st, a, m, t);
  else
    hipLaunchKernelGGL(k_cm_seg<false>, dim3(uint32_t(blocks)), dim3(THREADS), 0, st, a, m, t);
  return check_hip(hipGetLastError(), "k_cm_seg");
}

}  // extern "C"
