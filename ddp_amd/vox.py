"""Host layer of libddp_vox.so (include/ddp_vox_mi355x.h): the reference's ``Voxelization`` with a point and a voxel cap
(bev/mmdet3d/ops/voxel/voxelize.py, the sequential result of src/voxelization_cpu.cpp ``hard_voxelize_kernel``) and the batched form of
``BEVFusion.voxelize`` (bev/mmdet3d/models/fusion_models/bevfusion.py:135-163), on the device.

  ``grid_of``        the grid of ``Voxelization.__init__``: round((hi - lo) / vs) in fp32
  ``HardVoxelizer``  owns the workspace and the output buffers: ``cells`` / ``assign`` / ``assign_from_cells`` / ``tables`` only enqueue,
                     as do ``gather`` and ``pack``; ``voxelize`` and ``voxelize_batch`` run them and read the voxel counts once

There is no CPU fallback: CPU tensors raise.  The caller's points are only read.  Not built, refused by message: the dynamic path
(``max_num_points == -1`` or ``max_voxels == -1``, DynamicScatter), fp16 points, any backward.
"""
import ctypes as C

import torch

from . import _vox_lib as M
from .evaluation import _stream


def grid_of(voxel_size, point_cloud_range):
    """(3,) int64, as ``Voxelization.__init__`` forms it (voxelize.py:110-114)"""
    r = torch.tensor(point_cloud_range, dtype=torch.float32)
    v = torch.tensor(voxel_size, dtype=torch.float32)
    return torch.round((r[3:] - r[:3]) / v).long()


class HardVoxelizer:
    """One grid, one pair of caps.  A call with a new (B, Pmax, F) re-plans: the workspace and the output buffers grow as needed.  The
    tensors ``voxelize`` and ``voxelize_batch`` return are VIEWS of the owned buffers: the next call overwrites them."""

    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels):
        if int(max_num_points) == -1 or int(max_voxels) == -1:
            raise NotImplementedError('max_num_points == -1 or max_voxels == -1 is the dynamic path (DynamicScatter): not built')
        self.voxel_size = [float(v) for v in voxel_size]
        self.point_cloud_range = [float(v) for v in point_cloud_range]
        if len(self.voxel_size) != 3 or len(self.point_cloud_range) != 6:
            raise ValueError('voxel_size must have 3 entries and point_cloud_range 6')
        self.max_num_points, self.max_voxels = int(max_num_points), int(max_voxels)
        self.grid = [int(v) for v in grid_of(self.voxel_size, self.point_cloud_range)]
        self._shape = None            # (B, Pmax, F) of the tables in the workspace
        self._stage = None            # 'cells' | 'assigned'
        self._rows = self._counts = self._stride = None   # the points the tables were made of: alive while a captured graph may replay
        self._ws = None
        self._ws_given = False
        self._out = {}
        self.workspace_bytes(1, 1)    # refuse a grid or caps outside the library's limits here, not at the first call

    def cfg(self, batch, pmax, feats=3):
        return M.Cfg(int(batch), int(pmax), self.max_voxels, self.max_num_points, int(feats), (C.c_int32 * 3)(*self.grid),
                     (C.c_float * 3)(*self.point_cloud_range[:3]), (C.c_float * 3)(*self.voxel_size))

    def workspace_bytes(self, batch, pmax, feats=3):
        n = C.c_size_t(0)
        lib = M.load()
        M.check(lib.ddp_vox_workspace(C.byref(self.cfg(batch, pmax, feats)), C.byref(n)), lib)
        return int(n.value)

    def use_workspace(self, ws):
        """run in a caller's uint8 device buffer (256-byte aligned, at least ``workspace_bytes`` of every later call)"""
        if not torch.is_tensor(ws) or not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous():
            raise ValueError('the workspace must be a contiguous uint8 device tensor')
        if ws.data_ptr() % M.WS_ALIGN:
            raise ValueError(f'the workspace must be {M.WS_ALIGN}-byte aligned')
        self._ws, self._ws_given, self._shape, self._stage = ws, True, None, None
        return self

    def _workspace(self, shape, dev):
        need = self.workspace_bytes(*shape)
        if self._ws_given:
            if self._ws.numel() < need or self._ws.device != dev:
                raise ValueError(f'the given workspace holds {self._ws.numel()} bytes on {self._ws.device}, the call needs {need} on {dev}')
        elif self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws

    @staticmethod
    def _check_points(points):
        if torch.is_tensor(points):
            points = [points]
        if not isinstance(points, (list, tuple)) or not points:
            raise ValueError('points must be a (P, >= 3) tensor or a non-empty list of them, one per sample')
        rows, stride = [], None
        for b, p in enumerate(points):
            if torch.is_tensor(p) and p.dtype == torch.float16:
                raise NotImplementedError('fp16 points are not built: pass float32')
            if torch.is_tensor(p) and p.requires_grad:
                raise NotImplementedError('voxelisation has no backward: detach the points')
            if not torch.is_tensor(p) or not p.is_cuda:
                raise ValueError(f'points[{b}] must be a device tensor: ddp_amd.vox has no CPU path')
            if p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] < 3:
                raise ValueError(f'points[{b}] must be float32 of shape (P, >= 3), got {p.dtype} {tuple(p.shape)}')
            if stride is not None and int(p.shape[1]) != stride:
                raise ValueError('every sample of points must have the same number of columns')
            stride = int(p.shape[1])
            rows.append(p.contiguous())   # a copy only of a non-contiguous view; the caller's tensor is never written
        return rows, stride

    def _point_args(self):
        B = len(self._rows)
        ptrs = (C.c_void_p * B)(*[p.data_ptr() if n else None for p, n in zip(self._rows, self._counts)])
        return ptrs, (C.c_int32 * B)(*self._counts), self._stride

    def _take(self, points, pmax, feats=None):
        rows, stride = self._check_points(points)
        counts = [int(p.shape[0]) for p in rows]
        pmax = max(max(counts), 1) if pmax is None else int(pmax)
        shape = (len(rows), pmax, stride if feats is None else int(feats))
        ws = self._workspace(shape, rows[0].device)
        self._rows, self._counts, self._stride = rows, counts, stride
        return shape, ws

    def cells(self, points, pmax=None, feats=None):
        """``points``: a (P, >= 3) device fp32 tensor or a list of B of them (rows x, y, z, ...) -> the (B, Pmax) cell table in the
        workspace.  ``pmax``: rows the tables reserve per sample (default: the largest count, at least 1); ``feats``: the leading F <= 16
        columns that reach the outputs (default: all)."""
        shape, ws = self._take(points, pmax, feats)
        lib = M.load()
        M.check(lib.ddp_vox_cells(C.byref(self.cfg(*shape)), *self._point_args(), ws.data_ptr(), _stream(ws.device)), lib)
        self._shape, self._stage = shape, 'cells'
        return self

    def assign(self):
        """the cell table of ``cells`` -> the voxel tables"""
        if self._stage is None:
            raise RuntimeError('no cell table in the workspace: call cells() first')
        lib = M.load()
        M.check(lib.ddp_vox_assign(C.byref(self.cfg(*self._shape)), self._ws.data_ptr(), _stream(self._ws.device)), lib)
        self._stage = 'assigned'
        return self

    def assign_from_cells(self, table, points=None, feats=None):
        """the same from a caller's (B, Pmax) int32 cell table (an id outside [0, grid volume) counts as -1).  ``points``: the rows
        ``gather`` and ``pack`` read afterwards (without them only ``tables`` can follow)."""
        if not torch.is_tensor(table) or not table.is_cuda:
            raise ValueError('table must be a device tensor: ddp_amd.vox has no CPU path')
        if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] < 1:
            raise ValueError(f'table must be int32 of shape (B, Pmax >= 1), got {table.dtype} {tuple(table.shape)}')
        table = table.contiguous()
        B, pmax = (int(v) for v in table.shape)
        if points is not None:
            shape, ws = self._take(points, pmax, feats)
            if shape[0] != B:
                raise ValueError('points must hold one entry per row of table')
        else:
            shape = (B, pmax, 3)
            ws = self._workspace(shape, table.device)
            self._rows = self._counts = self._stride = None
        lib = M.load()
        M.check(lib.ddp_vox_assign_from_cells(C.byref(self.cfg(*shape)), table.data_ptr(), ws.data_ptr(), _stream(ws.device)), lib)
        self._shape, self._stage = shape, 'assigned'
        return self

    def tables(self):
        """views of the workspace, all int32: cells (B, Pmax), point_voxel (B, Pmax), voxel_points (B, max_voxels, T), voxel_cells
        (B, max_voxels), counts (B); what each holds: include/ddp_vox_mi355x.h ``ddp_vox_tables``"""
        if self._stage is None:
            raise RuntimeError('no tables in the workspace: call cells() first')
        B, pmax, F = self._shape
        lib = M.load()
        ptrs = [C.c_void_p(0) for _ in range(5)]
        M.check(lib.ddp_vox_tables(C.byref(self.cfg(B, pmax, F)), self._ws.data_ptr(), *[C.byref(p) for p in ptrs]), lib)
        base = self._ws.data_ptr()
        V, T = self.max_voxels, self.max_num_points
        shapes = [(B, pmax), (B, pmax), (B, V, T), (B, V), (B,)]

        def view(p, shape):
            n = 1
            for v in shape:
                n *= v
            return self._ws[p.value - base:p.value - base + 4 * n].view(torch.int32).view(shape)
        return tuple(view(p, s) for p, s in zip(ptrs, shapes))

    def _assigned(self):
        if self._stage != 'assigned':
            raise RuntimeError('no voxel tables in the workspace: call assign() first')
        if self._rows is None:
            raise RuntimeError('the voxel tables were made without points: pass points to assign_from_cells()')
        return self._shape

    def _buffers(self, kind, shapes, out):
        dev = self._ws.device
        dtypes = (torch.float32, torch.int32, torch.int32)
        if out is not None:
            for t, s, dt in zip(out, shapes, dtypes):
                if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dt or tuple(t.shape) != s or not t.is_contiguous():
                    raise ValueError(f'out must be contiguous device tensors of shapes {shapes} (float32, int32, int32)')
            return tuple(out)
        have = self._out.get(kind)
        if have is None or tuple(tuple(t.shape) for t in have) != shapes or have[0].device != dev:
            have = self._out[kind] = tuple(torch.empty(s, dtype=dt, device=dev) for s, dt in zip(shapes, dtypes))
        return have

    def gather(self, out=None):
        """-> voxels (B, max_voxels, T, F), coors (B, max_voxels, 3) x y z, num_points (B, max_voxels) at full capacity; rows >= M_b are
        left as they were.  Enqueues only."""
        B, pmax, F = self._assigned()
        V, T = self.max_voxels, self.max_num_points
        voxels, coors, num = self._buffers('gather', ((B, V, T, F), (B, V, 3), (B, V)), out)
        lib = M.load()
        M.check(lib.ddp_vox_gather(C.byref(self.cfg(B, pmax, F)), *self._point_args(), self._ws.data_ptr(), voxels.data_ptr(), coors.data_ptr(),
                                   num.data_ptr(), _stream(self._ws.device)), lib)
        return voxels, coors, num

    def pack(self, reduce=True, out=None):
        """-> feats (B * max_voxels, F) means, or (B * max_voxels, T, F) with ``reduce=False``, coords (B * max_voxels, 4) sample x y z,
        sizes (B * max_voxels) at full capacity; rows >= sum(M_b) are left as they were.  Enqueues only."""
        B, pmax, F = self._assigned()
        V, T = self.max_voxels, self.max_num_points
        shapes = ((B * V, F) if reduce else (B * V, T, F), (B * V, 4), (B * V,))
        feats, coords, sizes = self._buffers('pack' if reduce else 'pack_raw', shapes, out)
        lib = M.load()
        M.check(lib.ddp_vox_pack(C.byref(self.cfg(B, pmax, F)), *self._point_args(), 1 if reduce else 0, self._ws.data_ptr(), feats.data_ptr(),
                                 coords.data_ptr(), sizes.data_ptr(), _stream(self._ws.device)), lib)
        return feats, coords, sizes

    def counts(self):
        """the B voxel counts M_b as a list of ints: the one copy to the host, which waits for the launches before it"""
        return [int(v) for v in self.tables()[4].cpu()]

    def voxelize(self, points, out=None, feats=None):
        """one sample -> the reference's triple: voxels (M, T, F), coors (M, 3) int32 x y z, num_points (M) int32"""
        if not torch.is_tensor(points):
            raise ValueError('points must be one (P, >= 3) tensor: voxelize_batch takes a list')
        voxels, coors, num = self.cells(points, feats=feats).assign().gather(out)
        m = self.counts()[0]
        return voxels[0, :m], coors[0, :m], num[0, :m]

    def voxelize_batch(self, points, reduce=True, out=None, feats=None):
        """a list of B samples -> feats, coords (sum M, 4) int32 with the sample index in column 0, sizes (sum M) int32; ``feats`` is
        (sum M, F), the mean of a voxel's points, or with ``reduce=False`` the (sum M, T, F) rows"""
        if torch.is_tensor(points):
            raise ValueError('points must be a list of (P, >= 3) tensors, one per sample')
        rows, coords, sizes = self.cells(points, feats=feats).assign().pack(reduce, out)
        m = sum(self.counts())
        return rows[:m], coords[:m], sizes[:m]
