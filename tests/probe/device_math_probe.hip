// device_math_probe.hip - test-only probes of the elementwise __device__ functions of csrc/ (tests/test_device_math_gpu.py).
// One bounds-checked elementwise kernel per function under test: 256 threads per block, grid = ceil(n / 256), plain vector
// loads and stores, no LDS, no atomics.  Built by ddp_amd/build.py into ddp_amd/lib/libddp_probe.so; the package never loads it
// and libddp_mi355x.so does not contain it.
//
// Launchers: extern "C" int probe_*(const float* d_in, <outputs>, int n, void* stream): enqueue on the stream, allocate
// nothing, return the launch status (hipError_t as int).  Kernels that take 4 / 8 values per thread read elements past n as 0
// and write only elements below n; a packed word u of p1 / p2 / p3 holds elements 2u (low half) and 2u + 1 (high half), so the
// word arrays need (n + 1) / 2 entries.
#include <utility>

#include "ddp_internal.h"

#include "layer_bf16x3.h"

namespace {

using namespace ddp;
using namespace ddp::b3;

// ---- compile-time checks of the hand-kept scheduling tables: a violated invariant fails the build ----
constexpr bool gelu_sched_ok() {
  for (int v = 0; v < 4; ++v) {
    int next = 0;                                   // ops of one value: 0, 1, .., 17 in strictly increasing slot order.  The table
    for (int sl = 0; sl < 24; ++sl) {               // holds ONE op per value per slot by construction; each op exactly once
      const int op = GELU_SCHED[sl][v];             // and in order <=> the non-negative entries read 0, 1, .., GELU_OPS - 1
      if (op < -1 || op >= GELU_OPS) return false;
      if (op >= 0) {
        if (op != next) return false;
        ++next;
      }
    }
    if (next != GELU_OPS) return false;
  }
  return true;
}
constexpr bool gelu_sched_packs_after_ops() {       // slots 21..23 pack the pieces of all four values: no op may sit there or later
  for (int sl = 21; sl < 24; ++sl)
    for (int v = 0; v < 4; ++v)
      if (GELU_SCHED[sl][v] != -1) return false;
  return true;
}
constexpr bool split_hand_ok() {
  if (SPLIT_HAND_LO[0] != 0 || SPLIT_HAND_LO[12] != 44) return false;
  for (int k = 0; k < 12; ++k)
    if (SPLIT_HAND_LO[k + 1] <= SPLIT_HAND_LO[k]) return false;
  return true;
}
static_assert(sizeof(GELU_SCHED) == 24 * 4 * sizeof(int), "GELU_SCHED is [24 slots][4 values]");
static_assert(GELU_OPS == 18, "the probes run gelu_op<0> .. gelu_op<17>");
static_assert(gelu_sched_ok(), "GELU_SCHED: every op 0..17 of every value exactly once, in strictly increasing slot order");
static_assert(gelu_sched_packs_after_ops(), "GELU_SCHED: slots 21..23 carry the packs and no op");
static_assert(split_hand_ok(), "SPLIT_HAND_LO: strictly increasing from 0 to 44");

constexpr int PT = 256;

__device__ __forceinline__ long gid() { return long(blockIdx.x) * PT + threadIdx.x; }
__device__ __forceinline__ float ld(const float* in, long i, int n) { return i < n ? in[i] : 0.f; }

template <int... I>
__device__ __forceinline__ void gelu_all_ops(GeluState& g, float v, std::integer_sequence<int, I...>) {
  (gelu_op<I>(g, v), ...);
}

// p1 / p2 / p3 of eight values starting at element e0 -> the word arrays (element pairs below n only)
__device__ __forceinline__ void store_packed8(const u32x4& p1, const u32x4& p2, const u32x4& p3, unsigned* o1, unsigned* o2,
                                              unsigned* o3, long e0, int n) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long w = e0 / 2 + u;
    if (2 * w < n) {
      o1[w] = p1[u];
      o2[w] = p2[u];
      o3[w] = p3[u];
    }
  }
}

__global__ void __launch_bounds__(PT) k_probe_gelu_fast(const float* in, float* out, int n) {
  const long i = gid();
  if (i < n) out[i] = gelu_fast(in[i]);
}

__global__ void __launch_bounds__(PT) k_probe_sigmoid(const float* in, float* out, int n) {
  const long i = gid();
  if (i < n) out[i] = sigmoidf_(in[i]);
}

__global__ void __launch_bounds__(PT) k_probe_gelu_ops(const float* in, unsigned* ph, unsigned* pm, unsigned* pl, int n) {
  const long i = gid();
  if (i >= n) return;
  GeluState g;
  gelu_all_ops(g, in[i], std::make_integer_sequence<int, GELU_OPS>{});
  ph[i] = gelu_ph(g);
  pm[i] = gelu_pm(g);
  pl[i] = gelu_pl(g);
}

template <int... SL>
__device__ __forceinline__ void gelu_sched_slots(GeluState& g0, GeluState& g1, GeluState& g2, GeluState& g3, float v0, float v1,
                                                 float v2, float v3, std::integer_sequence<int, SL...>) {
  // one slot after the other, the four values inside a slot in the order of the fc2 loop (layer_bf16x3.h, P2)
  ((gelu_maybe<GELU_SCHED[SL][0]>(g0, v0), gelu_maybe<GELU_SCHED[SL][1]>(g1, v1), gelu_maybe<GELU_SCHED[SL][2]>(g2, v2),
    gelu_maybe<GELU_SCHED[SL][3]>(g3, v3)),
   ...);
}

__global__ void __launch_bounds__(PT) k_probe_gelu_sched(const float* in, unsigned* ph, unsigned* pm, unsigned* pl, int n) {
  const long e0 = gid() * 4;
  if (e0 >= n) return;
  GeluState g[4];
  gelu_sched_slots(g[0], g[1], g[2], g[3], ld(in, e0, n), ld(in, e0 + 1, n), ld(in, e0 + 2, n), ld(in, e0 + 3, n),
                   std::make_integer_sequence<int, 24>{});
#pragma unroll
  for (int v = 0; v < 4; ++v)
    if (e0 + v < n) {
      ph[e0 + v] = gelu_ph(g[v]);
      pm[e0 + v] = gelu_pm(g[v]);
      pl[e0 + v] = gelu_pl(g[v]);
    }
}

// MODE 0: gelu_split8_packed  1: split8  2: split8_packed  3: split_op over ops 0..43 grouped by SPLIT_HAND_LO
template <int MODE>
__global__ void __launch_bounds__(PT) k_probe_packed8(const float* in, unsigned* o1, unsigned* o2, unsigned* o3, int n) {
  const long e0 = gid() * 8;
  if (e0 >= n) return;
  float x[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = ld(in, e0 + e, n);
  u32x4 p[3];
  if constexpr (MODE == 0) gelu_split8_packed(x, p[0], p[1], p[2]);
  if constexpr (MODE == 1) split8(x, p[0], p[1], p[2]);
  if constexpr (MODE == 2) split8_packed(x, p[0], p[1], p[2]);
  if constexpr (MODE == 3) {
    const f32x4 a = {x[0], x[1], x[2], x[3]}, b = {x[4], x[5], x[6], x[7]};
    SplitState s;
#pragma unroll
    for (int k = 0; k < 12; ++k)
#pragma unroll
      for (int op = SPLIT_HAND_LO[k]; op < SPLIT_HAND_LO[k + 1]; ++op) split_op(op, s, a, b, p);
  }
  store_packed8(p[0], p[1], p[2], o1, o2, o3, e0, n);
}

inline unsigned blocks(int n) { return unsigned((long(n) + PT - 1) / PT); }

template <class K, class... A>
int launch(K kernel, int n, void* stream, A... args) {
  if (n < 0) return int(hipErrorInvalidValue);
  if (n == 0) return int(hipSuccess);
  hipLaunchKernelGGL(kernel, dim3(blocks(n)), dim3(PT), 0, static_cast<hipStream_t>(stream), args..., n);
  return int(hipGetLastError());
}

}  // namespace

#define PROBE_API extern "C" __attribute__((visibility("default")))

PROBE_API int probe_gelu_fast(const float* d_in, float* d_out, int n, void* stream) {
  return launch(k_probe_gelu_fast, n, stream, d_in, d_out);
}
PROBE_API int probe_sigmoid(const float* d_in, float* d_out, int n, void* stream) {
  return launch(k_probe_sigmoid, n, stream, d_in, d_out);
}
PROBE_API int probe_gelu_ops(const float* d_in, unsigned* d_ph, unsigned* d_pm, unsigned* d_pl, int n, void* stream) {
  return launch(k_probe_gelu_ops, n, stream, d_in, d_ph, d_pm, d_pl);
}
PROBE_API int probe_gelu_sched(const float* d_in, unsigned* d_ph, unsigned* d_pm, unsigned* d_pl, int n, void* stream) {
  return launch(k_probe_gelu_sched, n, stream, d_in, d_ph, d_pm, d_pl);
}
PROBE_API int probe_gelu_packed(const float* d_in, unsigned* d_p1, unsigned* d_p2, unsigned* d_p3, int n, void* stream) {
  return launch(k_probe_packed8<0>, n, stream, d_in, d_p1, d_p2, d_p3);
}
PROBE_API int probe_split8(const float* d_in, unsigned* d_p1, unsigned* d_p2, unsigned* d_p3, int n, void* stream) {
  return launch(k_probe_packed8<1>, n, stream, d_in, d_p1, d_p2, d_p3);
}
PROBE_API int probe_split8_packed(const float* d_in, unsigned* d_p1, unsigned* d_p2, unsigned* d_p3, int n, void* stream) {
  return launch(k_probe_packed8<2>, n, stream, d_in, d_p1, d_p2, d_p3);
}
PROBE_API int probe_split_ops(const float* d_in, unsigned* d_p1, unsigned* d_p2, unsigned* d_p3, int n, void* stream) {
  return launch(k_probe_packed8<3>, n, stream, d_in, d_p1, d_p2, d_p3);
}
