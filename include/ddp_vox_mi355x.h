/* ddp_vox_mi355x.h - C ABI of libddp_vox.so: the start of the reference's lidar branch (bev/mmdet3d/models/fusion_models/bevfusion.py
 * `BEVFusion.voxelize`: `Voxelization` with a point and a voxel cap, the batch column, `voxelize_reduce`) on the MI355X (gfx950).
 * The result is the SEQUENTIAL one of bev/mmdet3d/ops/voxel/src/voxelization_cpu.cpp `hard_voxelize_kernel`, exactly: voxels are
 * numbered by the index of their first point, a voxel keeps its first `max_points` points in index order, only the first
 * `max_voxels` distinct cells exist.  A library of its own: no part of the sampler ABI (ddp_mi355x.h) nor of the evaluation,
 * confusion-matrix, LSS or depth-LSS libraries, linked into none of them.
 *
 * Three halves, each checkable on its own:
 *   cells   (fp32 -> integers)  per point the cell id (x * grid_y + y) * grid_z + z it falls in, or -1
 *   assign  (integers)          per point its voxel, per voxel its first max_points point indices and its cell, per sample M_b
 *   gather / pack (copies, one fp32 sum)  the reference's per-sample outputs / the batched outputs of `BEVFusion.voxelize`
 *
 * Conventions (those of ddp_dlss_mi355x.h)
 *  - plain C.  Every pointer named `d_*` is a DEVICE pointer to a contiguous array, every pointer named `h_*` a HOST pointer; the
 *    caller owns every buffer; the library never allocates or frees device memory.
 *  - all work is enqueued on the `hipStream_t` passed as `void* stream` (0 = default stream); no host synchronisation; every
 *    entry point can be captured into a hipGraph (the host arrays are read during the call, the device pointers they hold are baked
 *    into the launches).  The voxel counts M_b stay on the device: gather and pack read them there, in stream order.
 *  - return value: DDP_VOX_OK (0) or a negative DDP_VOX_E_* code (the values of DDP_E_*); `ddp_vox_last_error()` gives a message
 *    (thread-local).  A refused call enqueues nothing.
 *  - every output is a function of the inputs alone: no output depends on the arrival order of an atomic nor on which slot of the
 *    hash table a cell landed in; two runs leave the same bytes, and a batched call equals per-sample calls.
 */
#ifndef DDP_VOX_MI355X_H
#define DDP_VOX_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the entry points declared here are exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define DDP_VOX_ABI_VERSION 1
#define DDP_VOX_WS_ALIGN 256
#define DDP_VOX_MAX_FEATS 16        /* F: floats of a point row that reach the outputs */
#define DDP_VOX_MAX_POINTS 256      /* T: points a voxel keeps */
#define DDP_VOX_SCAN_TILE 1024      /* points one block numbers; a sample of more points takes more than one block */
#define DDP_VOX_HASH_MULT 2654435761u

enum { DDP_VOX_OK = 0, DDP_VOX_E_BADCFG = -1, DDP_VOX_E_ALIGN = -2, DDP_VOX_E_LAUNCH = -3, DDP_VOX_E_NULL = -4 };

/* B samples of at most `pmax` points; `max_voxels` (the reference's cap of the mode in use), `max_points` (T, its max_num_points),
 * `feats` (F) floats per output row; the grid `grid[j] = round((hi[j] - lo[j]) / vs[j])` as the caller formed it (fp32, as
 * `Voxelization.__init__` does), its lower bounds `lo` and the voxel size `vs`, x y z. */
typedef struct ddp_vox_cfg {
  int32_t batch, pmax, max_voxels, max_points, feats;
  int32_t grid[3];
  float lo[3];
  float vs[3];
} ddp_vox_cfg;

const char* ddp_vox_last_error(void);
int ddp_vox_abi_version(void);

/* Limits, refused with DDP_VOX_E_BADCFG before any launch: batch, pmax, max_voxels, max_points, feats and every grid side >= 1
 * (max_points = -1 or max_voxels = -1, the reference's dynamic path, is refused by this rule: DynamicScatter is not built);
 * feats <= 16; max_points <= 256; grid volume < 2^31; B*pmax < 2^31; B*max_voxels*max_points < 2^31; B*H < 2^31 with H the hash
 * capacity below; every lo finite; every vs finite and > 0.  A NULL pointer is DDP_VOX_E_NULL; d_workspace not DDP_VOX_WS_ALIGN-byte
 * aligned, or any other pointer not 4-byte aligned, is DDP_VOX_E_ALIGN.
 *
 * The workspace is a function of (batch, pmax, max_voxels, max_points) alone - NOT of the grid volume.  With P = B*pmax,
 * H = the smallest power of two >= 2*pmax, V = B*max_voxels, nt = ceil(pmax / 1024) and r(n) = n rounded up to 256 bytes:
 *   r(4P) cells + r(4P) point voxels + r(4V*T) voxel points + r(4V) voxel cells + r(4B) counts            the caller-visible tables
 *   + r(4P) point slots + 3 * r(4*B*H) hash keys, first indices, slot voxels + r(4*B*nt) tile sums + r(4(B+1)) row offsets.
 * Nothing but the tables survives a call, and no call reads what it, or the call documented to run before it, did not write.
 *
 * The hash (documented so that colliding ids can be built): cell id c of a sample has the home slot
 *   (uint32(c) * 2654435761u) >> (32 - log2 H)
 * in that sample's table of H slots, and takes the first free slot at home, home + 1, ... (mod H). */
int ddp_vox_workspace(const ddp_vox_cfg* cfg, size_t* bytes);

/* ---- cells -------------------------------------------------------------------------------------------------------------
 * h_points: B device pointers (a host array) to the point rows of each sample, `stride` floats per row (>= feats; x, y, z first),
 * h_counts: B host row counts, 0 <= count <= pmax (a zero count needs no valid pointer and gives a sample without a voxel).  The
 * points are only read.  Per point and axis j, fp32, one rounding per operation:
 *   q_j = floor((p_j - lo_j) / vs_j)          a subtraction and a correctly rounded division: no reciprocal, no contraction
 *   in range iff 0 <= q_j < grid[j] on all three axes, compared as floats: NaN, +-inf and values beyond the int range fail; -0.0 is 0
 * Entry (b, p) of the (B, pmax) cell table is (x * grid[1] + y) * grid[2] + z, or -1; entries p >= count are -1. */
int ddp_vox_cells(const ddp_vox_cfg* cfg, const float* const* h_points, const int32_t* h_counts, int32_t stride, void* d_workspace,
                  void* stream);

/* ---- assign ------------------------------------------------------------------------------------------------------------
 * From the cell table that ddp_vox_cells left in d_workspace (same cfg).  Launches, for any B: clear, insert (hash: key by
 * atomicCAS, first index by atomicMin), three of the scan that numbers the founders (the points that are their cell's first),
 * and max_points rounds that fill one column of the voxel points each - 5 + max_points in all.  Round s gives every voxel the
 * smallest index above its entry of round s - 1 by one atomicMin per point still waiting: at most max_points * B * pmax
 * atomics whatever a voxel's population, never a pass that is quadratic in it. */
int ddp_vox_assign(const ddp_vox_cfg* cfg, void* d_workspace, void* stream);

/* The same from a caller's (B, pmax) int32 cell table (one launch more: the copy); an id outside [0, grid volume) counts as -1. */
int ddp_vox_assign_from_cells(const ddp_vox_cfg* cfg, const int32_t* d_cells, void* d_workspace, void* stream);

/* Where the tables lie in the workspace (host arithmetic only), all int32:
 *   d_cells        (B, pmax)                    the cell id of a point or -1
 *   d_point_voxel  (B, pmax)                    the voxel of a point or -1 (out of range, or its cell came after the voxel cap);
 *                                               a point beyond its voxel's point cap still names the voxel
 *   d_voxel_points (B, max_voxels, max_points)  ascending point indices, -1 = empty; rows >= M_b are all -1
 *   d_voxel_cells  (B, max_voxels)              the cell id of a voxel; rows >= M_b are not written
 *   d_counts       (B)                          M_b = min(distinct cells, max_voxels) */
int ddp_vox_tables(const ddp_vox_cfg* cfg, void* d_workspace, const int32_t** d_cells, const int32_t** d_point_voxel,
                   const int32_t** d_voxel_points, const int32_t** d_voxel_cells, const int32_t** d_counts);

/* ---- gather ------------------------------------------------------------------------------------------------------------
 * The reference's per-sample outputs at capacity max_voxels, from the tables of an assign call and the points it was made of:
 *   d_voxels (B, max_voxels, T, F) fp32    the first F floats of the kept rows; an unused slot is +0.0, written by this call
 *   d_coors  (B, max_voxels, 3) int32      x, y, z (the order the reference's fork stores)
 *   d_num_points (B, max_voxels) int32     min(population, T)
 * Rows >= M_b of sample b are left untouched.  A table entry >= count[b] (possible only after assign_from_cells) counts as empty.
 * One launch per sample with a point, two kinds of them (rows; coors and sizes). */
int ddp_vox_gather(const ddp_vox_cfg* cfg, const float* const* h_points, const int32_t* h_counts, int32_t stride, void* d_workspace,
                   float* d_voxels, int32_t* d_coors, int32_t* d_num_points, void* stream);

/* ---- pack --------------------------------------------------------------------------------------------------------------
 * The batched outputs of `BEVFusion.voxelize` at capacity B*max_voxels rows: sample b starts at row M_0 + ... + M_(b-1), read from
 * the device counts in stream order; rows >= M_0 + ... + M_(B-1) are left untouched.
 *   d_feats   reduce != 0: (rows, F)  (x_0 + x_1 + ... + x_(n-1)) / float(n), summed left to right in fp32, one rounding per
 *                                     operation, one true division
 *             reduce == 0: (rows, T, F)  the rows of gather
 *   d_coords  (rows, 4) int32  sample index, x, y, z
 *   d_sizes   (rows) int32     n = min(population, T) */
int ddp_vox_pack(const ddp_vox_cfg* cfg, const float* const* h_points, const int32_t* h_counts, int32_t stride, int32_t reduce,
                 void* d_workspace, float* d_feats, int32_t* d_coords, int32_t* d_sizes, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* DDP_VOX_MI355X_H */
