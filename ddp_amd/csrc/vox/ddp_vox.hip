// libddp_vox.so (include/ddp_vox_mi355x.h): hard voxelisation of lidar points with the reference's sequential result - cell ids, a
// hash table from cell to first point index, a scan that numbers the founders, max_points rounds of atomicMin that fill the voxel
// points column by column - and the per-sample and batched outputs.  DESIGN.md §8.5 has the design.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../../include/ddp_vox_mi355x.h"

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
  if (e == hipSuccess) return DDP_VOX_OK;
  return fail(DDP_VOX_E_LAUNCH, "%s: %s", what, hipGetErrorString(e));
}

constexpr int WAVE = 64;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int SCAN_TILE = DDP_VOX_SCAN_TILE;
constexpr int PER_THREAD = SCAN_TILE / THREADS;
static_assert(PER_THREAD * THREADS == SCAN_TILE, "a tile is a whole number of points per thread");
constexpr unsigned EMPTY = 0xFFFFFFFFu;  // a free column of the voxel points: -1 as the int32 the caller reads, the largest unsigned

// ---- derived sizes and the workspace ---------------------------------------------------------------------------------------------
struct Dims {
  int P, H, shift, V, VT, nt, volume;  // points, hash slots per sample and 32 - log2 H, voxels, voxel point entries, scan tiles per sample
};

struct Carve {
  int *cells, *pvox, *vcell, *counts, *pslot, *keys, *vals, *svox, *sums, *offs;
  unsigned* table;
  size_t bytes;
};

size_t round_up(size_t n) { return (n + (DDP_VOX_WS_ALIGN - 1)) / DDP_VOX_WS_ALIGN * DDP_VOX_WS_ALIGN; }

Carve carve(const ddp_vox_cfg* cfg, const Dims& d, void* ws) {
  char* p = static_cast<char*>(ws);
  size_t o = 0;
  Carve c;
  auto take = [&](size_t n) { char* q = p + o; o += round_up(4 * n); return reinterpret_cast<int*>(q); };
  const size_t B = size_t(cfg->batch);
  c.cells = take(d.P);
  c.pvox = take(d.P);
  c.table = reinterpret_cast<unsigned*>(take(d.VT));
  c.vcell = take(d.V);
  c.counts = take(B);
  c.pslot = take(d.P);
  c.keys = take(B * d.H);
  c.vals = take(B * d.H);
  c.svox = take(B * d.H);
  c.sums = take(B * d.nt);
  c.offs = take(B + 1);
  c.bytes = o;
  return c;
}

int check_cfg(const ddp_vox_cfg* cfg, Dims* out) {
  if (!cfg) return fail(DDP_VOX_E_NULL, "cfg is NULL");
  const int ext[] = {cfg->batch, cfg->pmax, cfg->max_voxels, cfg->max_points, cfg->feats, cfg->grid[0], cfg->grid[1], cfg->grid[2]};
  const char* names[] = {"batch", "pmax", "max_voxels", "max_points", "feats", "grid[0]", "grid[1]", "grid[2]"};
  for (int i = 0; i < 8; ++i)
    if (ext[i] < 1)
      return fail(DDP_VOX_E_BADCFG, "extent %s = %d must be positive%s", names[i], ext[i],
                  (i == 2 || i == 3) && ext[i] == -1 ? " (-1 is the dynamic path, DynamicScatter: not built)" : "");
  if (cfg->feats > DDP_VOX_MAX_FEATS) return fail(DDP_VOX_E_BADCFG, "feats = %d exceeds %d", cfg->feats, DDP_VOX_MAX_FEATS);
  if (cfg->max_points > DDP_VOX_MAX_POINTS) return fail(DDP_VOX_E_BADCFG, "max_points = %d exceeds %d", cfg->max_points, DDP_VOX_MAX_POINTS);
  for (int j = 0; j < 3; ++j) {
    if (!std::isfinite(cfg->lo[j])) return fail(DDP_VOX_E_BADCFG, "lo[%d] must be finite", j);
    if (!std::isfinite(cfg->vs[j]) || !(cfg->vs[j] > 0.f)) return fail(DDP_VOX_E_BADCFG, "vs[%d] must be finite and positive", j);
  }
  const long long lim = 1ll << 31;
  const long long volume = (long long)cfg->grid[0] * cfg->grid[1];
  if (volume >= lim || volume * cfg->grid[2] >= lim) return fail(DDP_VOX_E_BADCFG, "grid too large: the grid volume must stay below 2^31");
  const long long B = cfg->batch;
  if (B * cfg->pmax >= lim) return fail(DDP_VOX_E_BADCFG, "too many points: B*pmax must stay below 2^31");
  if (B * cfg->max_voxels >= lim || B * cfg->max_voxels * cfg->max_points >= lim)
    return fail(DDP_VOX_E_BADCFG, "too many voxel points: B*max_voxels*max_points must stay below 2^31");
  long long H = 2;
  int log2H = 1;
  while (H < 2ll * cfg->pmax) {
    H <<= 1;
    ++log2H;
  }
  if (B * H >= lim) return fail(DDP_VOX_E_BADCFG, "hash table too large: B*H must stay below 2^31 (H = %lld slots per sample)", H);
  if (out) {
    out->P = int(B * cfg->pmax);
    out->H = int(H);
    out->shift = 32 - log2H;
    out->V = int(B * cfg->max_voxels);
    out->VT = int(B * cfg->max_voxels * cfg->max_points);
    out->nt = (cfg->pmax + SCAN_TILE - 1) / SCAN_TILE;
    out->volume = int(volume * cfg->grid[2]);
  }
  return DDP_VOX_OK;
}

int check_ptr(const void* p, const char* name, unsigned align) {
  if (!p) return fail(DDP_VOX_E_NULL, "%s is NULL", name);
  if (reinterpret_cast<uintptr_t>(p) & (align - 1)) return fail(DDP_VOX_E_ALIGN, "%s must be %u-byte aligned", name, align);
  return DDP_VOX_OK;
}

int check_points(const ddp_vox_cfg* cfg, const float* const* h_points, const int32_t* h_counts, int stride) {
  if (stride < cfg->feats) return fail(DDP_VOX_E_BADCFG, "stride = %d floats per point row must be at least feats = %d", stride, cfg->feats);
  if (cfg->feats < 3) return fail(DDP_VOX_E_BADCFG, "feats = %d: a point row starts with x, y, z", cfg->feats);
  if (!h_points) return fail(DDP_VOX_E_NULL, "h_points is NULL");
  if (!h_counts) return fail(DDP_VOX_E_NULL, "h_counts is NULL");
  for (int b = 0; b < cfg->batch; ++b) {
    if (h_counts[b] < 0) return fail(DDP_VOX_E_BADCFG, "count[%d] = %d must not be negative", b, h_counts[b]);
    if (h_counts[b] > cfg->pmax) return fail(DDP_VOX_E_BADCFG, "count[%d] = %d exceeds pmax = %d", b, h_counts[b], cfg->pmax);
    if (h_counts[b] > 0)
      if (int rc = check_ptr(h_points[b], "h_points[b]", 4)) return rc;
  }
  return DDP_VOX_OK;
}

unsigned blocks_for(long long n) { return unsigned((n + THREADS - 1) / THREADS); }

// ---- cells ------------------------------------------------------------------------------------------------------------------------
struct Geo {
  float lo[3], vs[3];
  int g[3];
};

// One sample: thread p is point p.  floor((p - lo) / vs) per axis, fp32, a subtraction and a true division; compared as floats.
__global__ void __launch_bounds__(THREADS) k_vox_cells(int pmax, int count, int stride, const Geo geo, const float* __restrict__ points,
                                                        int* __restrict__ cells) {
  const long long p_ll = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (p_ll >= pmax) return;
  const int p = int(p_ll);
  if (p >= count) {
    cells[p] = -1;
    return;
  }
  const float* q = points + (size_t)p * stride;
  int c[3];
  bool in = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float f = floorf(__fdiv_rn(__fsub_rn(q[j], geo.lo[j]), geo.vs[j]));
    in = in && f >= 0.f && f < float(geo.g[j]);  // NaN and +-inf fail; -0.0 passes and converts to 0
    c[j] = in ? int(f) : 0;
  }
  cells[p] = in ? (c[0] * geo.g[1] + c[1]) * geo.g[2] + c[2] : -1;  // < volume < 2^31
}

// a caller's table: an id outside [0, volume) counts as -1
__global__ void __launch_bounds__(THREADS) k_vox_take_cells(int P, int volume, const int* __restrict__ src, int* __restrict__ cells) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i >= P) return;
  const int c = src[i];
  cells[i] = c >= 0 && c < volume ? c : -1;
}

// ---- assign: cell -> first point index ----------------------------------------------------------------------------------------------
// A minimum only falls.  A load that sees a value <= v shows that v cannot win, however stale it is, so the atomic is skipped: of the
// thousands of points a crowded cell holds, only those that arrive before a smaller index go to the one address.
__device__ __forceinline__ void vox_min(int* addr, int v) {
  if (v < __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(addr, v);
}

__device__ __forceinline__ void vox_min(unsigned* addr, unsigned v) {
  if (v < __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(addr, v);
}

__global__ void __launch_bounds__(THREADS) k_vox_clear(int BH, int VT, int* __restrict__ keys, int* __restrict__ vals,
                                                        unsigned* __restrict__ table) {
  const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (i < BH) {
    keys[i] = -1;
    vals[i] = INT_MAX;
  }
  if (i < VT) table[i] = EMPTY;
}

// thread t = b * pmax + p.  A key, once set, never changes: a plain load that sees it is as good as the atomic; a plain load that
// sees a stale -1 goes on to the atomicCAS, which returns what the slot holds.  At most pmax of the H >= 2 * pmax slots are taken.
__global__ void __launch_bounds__(THREADS) k_vox_insert(int P, int pmax, int H, int shift, const int* __restrict__ cells,
                                                         int* __restrict__ keys, int* __restrict__ vals, int* __restrict__ pslot) {
  const long long t_ll = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (t_ll >= P) return;
  const int t = int(t_ll);
  const int c = cells[t];
  if (c < 0) {
    pslot[t] = -1;
    return;
  }
  const int b = t / pmax;
  int* kb = keys + (size_t)b * H;
  unsigned h = (unsigned(c) * DDP_VOX_HASH_MULT) >> shift;
  int found = -1;
  for (int probe = 0; probe < H; ++probe) {
    int k = kb[h];
    if (k == -1) k = atomicCAS(&kb[h], -1, c);
    if (k == -1 || k == c) {
      found = int(h);
      break;
    }
    h = (h + 1) & unsigned(H - 1);
  }
  pslot[t] = found;  // never -1 here: the table cannot fill
  if (found >= 0) vox_min(&vals[(size_t)b * H + found], t - b * pmax);
}

// ---- assign: number the founders ------------------------------------------------------------------------------------------------------
// A founder is the first point of its cell.  The exclusive scan of the founder flags over a sample's points, in three launches: a
// block sums a tile of SCAN_TILE flags; one block per sample scans the tile sums; a block scans its tile again, adds the tile's start
// and writes, per founder, the voxel of its slot and the cell of its voxel.
__device__ __forceinline__ int vox_founder(int p, int pmax, int b, int H, const int* __restrict__ pslot, const int* __restrict__ vals) {
  if (p >= pmax) return 0;
  const int s = pslot[(size_t)b * pmax + p];
  return s >= 0 && vals[(size_t)b * H + s] == p ? 1 : 0;
}

// inclusive scan of one value per thread over the block -> the thread's EXCLUSIVE prefix; *total = the block's sum
__device__ __forceinline__ int vox_block_excl(int v, int* wsum, int* total) {
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

// block b * nt + tile
__global__ void __launch_bounds__(THREADS) k_vox_tile_sums(int pmax, int H, int nt, const int* __restrict__ pslot,
                                                            const int* __restrict__ vals, int* __restrict__ sums) {
  __shared__ int wsum[WAVES];
  const int b = blockIdx.x / nt, tile = blockIdx.x - b * nt;
  const int p0 = tile * SCAN_TILE + threadIdx.x * PER_THREAD;  // < pmax + SCAN_TILE, and pmax <= 2^29 (B*H < 2^31)
  int n = 0;
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) n += vox_founder(p0 + k, pmax, b, H, pslot, vals);
  int total;
  vox_block_excl(n, wsum, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// block b: in-place exclusive scan of the sample's nt tile sums; counts[b] = min(their sum, max_voxels)
__global__ void __launch_bounds__(THREADS) k_vox_scan_sums(int nt, int max_voxels, int* __restrict__ sums, int* __restrict__ counts) {
  __shared__ int part[THREADS];
  const int tid = threadIdx.x;
  int* v = sums + (size_t)blockIdx.x * nt;
  const int per = (nt + THREADS - 1) / THREADS;
  const int lo = tid * per < nt ? tid * per : nt;
  const int hi = lo + per < nt ? lo + per : nt;
  int s = 0;
  for (int i = lo; i < hi; ++i) s += v[i];
  part[tid] = s;
  __syncthreads();
  for (int d = 1; d < THREADS; d <<= 1) {
    const int t = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += t;
    __syncthreads();
  }
  int run = part[tid] - s;
  for (int i = lo; i < hi; ++i) {
    const int c = v[i];
    v[i] = run;
    run += c;
  }
  if (tid == THREADS - 1) counts[blockIdx.x] = part[tid] < max_voxels ? part[tid] : max_voxels;
}

// block b * nt + tile
__global__ void __launch_bounds__(THREADS) k_vox_number(int pmax, int H, int nt, int max_voxels, const int* __restrict__ cells,
                                                         const int* __restrict__ pslot, const int* __restrict__ vals,
                                                         const int* __restrict__ sums, int* __restrict__ svox, int* __restrict__ vcell) {
  __shared__ int wsum[WAVES];
  const int b = blockIdx.x / nt, tile = blockIdx.x - b * nt;
  const int p0 = tile * SCAN_TILE + threadIdx.x * PER_THREAD;
  int f[PER_THREAD], n = 0;
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) {
    f[k] = vox_founder(p0 + k, pmax, b, H, pslot, vals);
    n += f[k];
  }
  int total;
  int v = sums[blockIdx.x] + vox_block_excl(n, wsum, &total);
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) {
    if (f[k]) {
      const size_t i = (size_t)b * pmax + p0 + k;
      const bool kept = v < max_voxels;
      svox[(size_t)b * H + pslot[i]] = kept ? v : -1;
      if (kept) vcell[(size_t)b * max_voxels + v] = cells[i];
      ++v;
    }
  }
}

// ---- assign: the first T points of a voxel ----------------------------------------------------------------------------------------------
// Round 0 also writes the point's voxel.  Round s > 0: a point above its voxel's entry of round s - 1 offers itself to column s; the
// minimum is the same whatever order the atomics arrive in.  A voxel whose column s - 1 stayed empty has no more points.
__global__ void __launch_bounds__(THREADS) k_vox_round0(int P, int pmax, int H, int max_voxels, int T, const int* __restrict__ pslot,
                                                         const int* __restrict__ svox, int* __restrict__ pvox, unsigned* __restrict__ table) {
  const long long t_ll = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (t_ll >= P) return;
  const int t = int(t_ll);
  const int b = t / pmax;
  const int s = pslot[t];
  const int v = s >= 0 ? svox[(size_t)b * H + s] : -1;  // -1 or < max_voxels: what k_vox_number wrote
  pvox[t] = v;
  if (v >= 0) vox_min(&table[((size_t)b * max_voxels + v) * T], unsigned(t - b * pmax));
}

__global__ void __launch_bounds__(THREADS) k_vox_round(int P, int pmax, int max_voxels, int T, int s, const int* __restrict__ pvox,
                                                        unsigned* __restrict__ table) {
  const long long t_ll = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (t_ll >= P) return;
  const int t = int(t_ll);
  const int v = pvox[t];
  if (v < 0) return;
  const int b = t / pmax;
  const unsigned p = unsigned(t - b * pmax);
  unsigned* row = table + ((size_t)b * max_voxels + v) * T;
  const unsigned prev = row[s - 1];
  if (prev == EMPTY || p <= prev) return;
  vox_min(&row[s], p);
}

// ---- gather and pack ------------------------------------------------------------------------------------------------------------------
// One sample.  Thread t is float f of slot s of voxel v: consecutive lanes read consecutive floats of one point row and write
// consecutive floats of the output.  `offs`: NULL (gather) or the sample's first row in the batched output (pack).
__global__ void __launch_bounds__(THREADS) k_vox_rows(int max_voxels, int T, int F, int stride, int count, const float* __restrict__ points,
                                                       const unsigned* __restrict__ table, const int* __restrict__ m, const int* __restrict__ offs,
                                                       float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
  const int TF = T * F;
  if (t >= (long long)max_voxels * TF) return;
  const int v = int(t / TF);
  if (v >= *m) return;
  const int r = int(t - (long long)v * TF);
  const int s = r / F, f = r - s * F;
  const unsigned idx = table[(size_t)v * T + s];
  const size_t row = (offs ? size_t(*offs) : 0) + v;
  out[row * TF + r] = idx < unsigned(count) ? points[(size_t)idx * stride + f] : 0.f;  // EMPTY is above every count
}

// thread v: the voxel's coordinates (`cols` = 3: x y z; 4: sample x y z) and its point count
__global__ void __launch_bounds__(THREADS) k_vox_meta(int max_voxels, int T, int gy, int gz, int count, int cols, int sample,
                                                       const unsigned* __restrict__ table, const int* __restrict__ vcell,
                                                       const int* __restrict__ m, const int* __restrict__ offs, int* __restrict__ coors,
                                                       int* __restrict__ sizes) {
  const long long v_ll = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (v_ll >= max_voxels) return;
  const int v = int(v_ll);
  if (v >= *m) return;
  int n = 0;
  while (n < T && table[(size_t)v * T + n] < unsigned(count)) ++n;
  const int c = vcell[v];
  const int z = c % gz, xy = c / gz;
  const size_t row = (offs ? size_t(*offs) : 0) + v;
  int* dst = coors + row * cols;
  if (cols == 4) *dst++ = sample;
  dst[0] = xy / gy;
  dst[1] = xy % gy;
  dst[2] = z;
  sizes[row] = n;
}

// thread t is float f of voxel v: the mean of its n kept rows, summed left to right, one rounding per operation, one true division
__global__ void __launch_bounds__(THREADS) k_vox_mean(int max_voxels, int T, int F, int stride, int count, const float* __restrict__ points,
                                                       const unsigned* __restrict__ table, const int* __restrict__ m, const int* __restrict__ offs,
                                                       float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (t >= (long long)max_voxels * F) return;
  const int v = int(t / F);
  if (v >= *m) return;
  const int f = int(t - (long long)v * F);
  float sum = 0.f;
  int n = 0;
  for (; n < T; ++n) {
    const unsigned idx = table[(size_t)v * T + n];
    if (idx >= unsigned(count)) break;
    const float x = points[(size_t)idx * stride + f];
    sum = n ? __fadd_rn(sum, x) : x;
  }
  out[(size_t(*offs) + v) * F + f] = __fdiv_rn(sum, float(n));
}

// one thread: offs[b] = M_0 + ... + M_(b-1)
__global__ void k_vox_offsets(int B, const int* __restrict__ counts, int* __restrict__ offs) {
  if (blockIdx.x || threadIdx.x) return;
  int run = 0;
  for (int b = 0; b < B; ++b) {
    offs[b] = run;
    run += counts[b];
  }
  offs[B] = run;
}

int run_assign(const ddp_vox_cfg* cfg, const Dims& d, const Carve& w, hipStream_t st) {
  const int B = cfg->batch, T = cfg->max_points, V = cfg->max_voxels, BH = B * d.H;
  hipLaunchKernelGGL(k_vox_clear, dim3(blocks_for(BH > d.VT ? BH : d.VT)), dim3(THREADS), 0, st, BH, d.VT, w.keys, w.vals, w.table);
  hipLaunchKernelGGL(k_vox_insert, dim3(blocks_for(d.P)), dim3(THREADS), 0, st, d.P, cfg->pmax, d.H, d.shift, w.cells, w.keys, w.vals, w.pslot);
  hipLaunchKernelGGL(k_vox_tile_sums, dim3(unsigned(B * d.nt)), dim3(THREADS), 0, st, cfg->pmax, d.H, d.nt, w.pslot, w.vals, w.sums);
  hipLaunchKernelGGL(k_vox_scan_sums, dim3(B), dim3(THREADS), 0, st, d.nt, V, w.sums, w.counts);
  hipLaunchKernelGGL(k_vox_number, dim3(unsigned(B * d.nt)), dim3(THREADS), 0, st, cfg->pmax, d.H, d.nt, V, w.cells, w.pslot, w.vals, w.sums, w.svox, w.vcell);
  hipLaunchKernelGGL(k_vox_round0, dim3(blocks_for(d.P)), dim3(THREADS), 0, st, d.P, cfg->pmax, d.H, V, T, w.pslot, w.svox, w.pvox, w.table);
  for (int s = 1; s < T; ++s)
    hipLaunchKernelGGL(k_vox_round, dim3(blocks_for(d.P)), dim3(THREADS), 0, st, d.P, cfg->pmax, V, T, s, w.pvox, w.table);
  return check_hip(hipGetLastError(), "assign kernels");
}

}  // namespace

extern "C" {

const char* ddp_vox_last_error(void) { return g_err; }

int ddp_vox_abi_version(void) { return DDP_VOX_ABI_VERSION; }

int ddp_vox_workspace(const ddp_vox_cfg* cfg, size_t* bytes) {
  if (!bytes) return fail(DDP_VOX_E_NULL, "bytes is NULL");
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  *bytes = carve(cfg, d, nullptr).bytes;
  return DDP_VOX_OK;
}

int ddp_vox_tables(const ddp_vox_cfg* cfg, void* d_workspace, const int32_t** d_cells, const int32_t** d_point_voxel,
                   const int32_t** d_voxel_points, const int32_t** d_voxel_cells, const int32_t** d_counts) {
  if (!d_cells) return fail(DDP_VOX_E_NULL, "d_cells is NULL");
  if (!d_point_voxel) return fail(DDP_VOX_E_NULL, "d_point_voxel is NULL");
  if (!d_voxel_points) return fail(DDP_VOX_E_NULL, "d_voxel_points is NULL");
  if (!d_voxel_cells) return fail(DDP_VOX_E_NULL, "d_voxel_cells is NULL");
  if (!d_counts) return fail(DDP_VOX_E_NULL, "d_counts is NULL");
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_VOX_WS_ALIGN)) return rc;
  const Carve w = carve(cfg, d, d_workspace);
  *d_cells = w.cells;
  *d_point_voxel = w.pvox;
  *d_voxel_points = reinterpret_cast<const int32_t*>(w.table);
  *d_voxel_cells = w.vcell;
  *d_counts = w.counts;
  return DDP_VOX_OK;
}

int ddp_vox_cells(const ddp_vox_cfg* cfg, const float* const* h_points, const int32_t* h_counts, int32_t stride, void* d_workspace,
                  void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_points(cfg, h_points, h_counts, stride)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_VOX_WS_ALIGN)) return rc;
  const Carve w = carve(cfg, d, d_workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  Geo geo;
  for (int j = 0; j < 3; ++j) {
    geo.lo[j] = cfg->lo[j];
    geo.vs[j] = cfg->vs[j];
    geo.g[j] = cfg->grid[j];
  }
  for (int b = 0; b < cfg->batch; ++b)
    hipLaunchKernelGGL(k_vox_cells, dim3(blocks_for(cfg->pmax)), dim3(THREADS), 0, st, cfg->pmax, h_counts[b], stride, geo, h_points[b],
                       w.cells + (size_t)b * cfg->pmax);
  return check_hip(hipGetLastError(), "cell kernels");
}

int ddp_vox_assign(const ddp_vox_cfg* cfg, void* d_workspace, void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_VOX_WS_ALIGN)) return rc;
  return run_assign(cfg, d, carve(cfg, d, d_workspace), static_cast<hipStream_t>(stream));
}

int ddp_vox_assign_from_cells(const ddp_vox_cfg* cfg, const int32_t* d_cells, void* d_workspace, void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_ptr(d_cells, "d_cells", 4)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_VOX_WS_ALIGN)) return rc;
  const Carve w = carve(cfg, d, d_workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_vox_take_cells, dim3(blocks_for(d.P)), dim3(THREADS), 0, st, d.P, d.volume, d_cells, w.cells);
  return run_assign(cfg, d, w, st);
}

int ddp_vox_gather(const ddp_vox_cfg* cfg, const float* const* h_points, const int32_t* h_counts, int32_t stride, void* d_workspace,
                   float* d_voxels, int32_t* d_coors, int32_t* d_num_points, void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_points(cfg, h_points, h_counts, stride)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_VOX_WS_ALIGN)) return rc;
  if (int rc = check_ptr(d_voxels, "d_voxels", 4)) return rc;
  if (int rc = check_ptr(d_coors, "d_coors", 4)) return rc;
  if (int rc = check_ptr(d_num_points, "d_num_points", 4)) return rc;
  const Carve w = carve(cfg, d, d_workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int V = cfg->max_voxels, T = cfg->max_points, F = cfg->feats;
  for (int b = 0; b < cfg->batch; ++b) {
    if (h_counts[b] == 0) continue;  // M_b = 0: no row to write
    const unsigned* table = w.table + (size_t)b * V * T;
    hipLaunchKernelGGL(k_vox_rows, dim3(blocks_for((long long)V * T * F)), dim3(THREADS), 0, st, V, T, F, stride, h_counts[b], h_points[b], table,
                       w.counts + b, (const int*)nullptr, d_voxels + (size_t)b * V * T * F);
    hipLaunchKernelGGL(k_vox_meta, dim3(blocks_for(V)), dim3(THREADS), 0, st, V, T, cfg->grid[1], cfg->grid[2], h_counts[b], 3, b, table,
                       w.vcell + (size_t)b * V, w.counts + b, (const int*)nullptr, d_coors + (size_t)b * V * 3, d_num_points + (size_t)b * V);
  }
  return check_hip(hipGetLastError(), "gather kernels");
}

int ddp_vox_pack(const ddp_vox_cfg* cfg, const float* const* h_points, const int32_t* h_counts, int32_t stride, int32_t reduce,
                 void* d_workspace, float* d_feats, int32_t* d_coords, int32_t* d_sizes, void* stream) {
  Dims d;
  if (int rc = check_cfg(cfg, &d)) return rc;
  if (int rc = check_points(cfg, h_points, h_counts, stride)) return rc;
  if (int rc = check_ptr(d_workspace, "d_workspace", DDP_VOX_WS_ALIGN)) return rc;
  if (int rc = check_ptr(d_feats, "d_feats", 4)) return rc;
  if (int rc = check_ptr(d_coords, "d_coords", 4)) return rc;
  if (int rc = check_ptr(d_sizes, "d_sizes", 4)) return rc;
  const Carve w = carve(cfg, d, d_workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int V = cfg->max_voxels, T = cfg->max_points, F = cfg->feats;
  hipLaunchKernelGGL(k_vox_offsets, dim3(1), dim3(WAVE), 0, st, cfg->batch, w.counts, w.offs);
  for (int b = 0; b < cfg->batch; ++b) {
    if (h_counts[b] == 0) continue;
    const unsigned* table = w.table + (size_t)b * V * T;
    if (reduce)
      hipLaunchKernelGGL(k_vox_mean, dim3(blocks_for((long long)V * F)), dim3(THREADS), 0, st, V, T, F, stride, h_counts[b], h_points[b], table,
                         w.counts + b, w.offs + b, d_feats);
    else
      hipLaunchKernelGGL(k_vox_rows, dim3(blocks_for((long long)V * T * F)), dim3(THREADS), 0, st, V, T, F, stride, h_counts[b], h_points[b],
                         table, w.counts + b, w.offs + b, d_feats);
    hipLaunchKernelGGL(k_vox_meta, dim3(blocks_for(V)), dim3(THREADS), 0, st, V, T, cfg->grid[1], cfg->grid[2], h_counts[b], 4, b, table,
                       w.vcell + (size_t)b * V, w.counts + b, w.offs + b, d_coords, d_sizes);
  }
  return check_hip(hipGetLastError(), "pack kernels");
}

}  // extern "C"
