"""Host layer of libddp_lss.so (include/ddp_lss_mi355x.h): the lift and pool of the reference's ``LSSTransform``
(bev/mmdet3d/models/vtransforms/base.py ``get_geometry`` + ``bev_pool``, lss.py ``get_cam_feats``) on the device, without the
(B, N, D, fH, fW, C) volume.

  ``grid_of``     dx, bx, nx by the reference's own expressions (``gen_dx_bx``), ``depth_bins_of`` the reference's D
  ``pack_cameras``  the (B, N, 24) / (B, 12) matrix tables of one sample batch: the 3 x 3 inverses and the one product stay torch ops
  ``LssPool``     owns the workspace: ``plan`` / ``plan_from_ranks`` / ``ranks`` / ``pool``

There is no CPU fallback: CPU tensors raise.
"""
import ctypes as C

import torch

from . import _lss_lib as M
from .evaluation import _stream


def grid_of(xbound, ybound, zbound):
    """base.py:12-18 ``gen_dx_bx``, the same expressions: nx is a Python-float division truncated by ``torch.LongTensor``"""
    dx = torch.Tensor([row[2] for row in [xbound, ybound, zbound]])
    bx = torch.Tensor([row[0] + row[2] / 2.0 for row in [xbound, ybound, zbound]])
    nx = torch.LongTensor([(row[1] - row[0]) / row[2] for row in [xbound, ybound, zbound]])
    return dx, bx, nx


def depth_bins_of(dbound):
    """D of base.py:57-62: the length of ``torch.arange(*dbound, dtype=torch.float)``"""
    return int(torch.arange(*dbound, dtype=torch.float).shape[0])


def pack_cameras(camera2lidar_rots, camera2lidar_trans, intrins, post_rots, post_trans, extra_rots, extra_trans):
    """-> cam (B, N, 24), extra (B, 12) fp32, where the inputs live: inverse(post_rot) 9, post_trans 3,
    combine = camera2lidar_rot @ inverse(intrins) 9, camera2lidar_trans 3; extra_rot 9, extra_trans 3 (base.py:92-108)."""
    B, N, _ = camera2lidar_trans.shape
    inv_post = torch.inverse(post_rots)
    combine = camera2lidar_rots.matmul(torch.inverse(intrins))
    cam = torch.cat([inv_post.reshape(B, N, 9), post_trans.reshape(B, N, 3), combine.reshape(B, N, 9),
                     camera2lidar_trans.reshape(B, N, 3)], dim=2).float().contiguous()
    extra = torch.cat([extra_rots.reshape(B, 9), extra_trans.reshape(B, 3)], dim=1).float().contiguous()
    return cam, extra


def _dev_f32(t, what, shape=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f'{what} must be a device tensor: ddp_amd.lss has no CPU path')
    if t.dtype != torch.float32:
        raise ValueError(f'{what} must be float32, got {t.dtype}')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'{what} must have shape {tuple(shape)}, got {tuple(t.shape)}')
    return t.contiguous()


class LssPool:
    """The device lift and pool of one ``LSSTransform`` geometry.  ``plan`` (or ``plan_from_ranks``) fixes batch and cameras and
    leaves the plan in the workspace this object owns; ``pool`` uses it.  Nothing synchronises."""

    def __init__(self, image_size, feature_size, xbound, ybound, zbound, dbound, channels):
        self.image_size = tuple(int(v) for v in image_size)
        self.feature_size = tuple(int(v) for v in feature_size)
        self.bounds = [tuple(float(v) for v in b) for b in (dbound, xbound, ybound, zbound)]
        self.C = int(channels)
        self.D = depth_bins_of(dbound)
        self.nx = [int(v) for v in grid_of(xbound, ybound, zbound)[2]]
        self._shape = None            # (B, N) of the plan in the workspace
        self._ws = None
        self._ws_given = False
        self.cfg(1, 1, check=True)    # refuse a geometry outside the library's limits here, not at the first call

    def cfg(self, batch, cams, check=False):
        c = M.Cfg(int(batch), int(cams), self.D, self.feature_size[0], self.feature_size[1], self.C, self.image_size[0], self.image_size[1])
        for name, b in zip(('dbound', 'xbound', 'ybound', 'zbound'), self.bounds):
            getattr(c, name)[:] = b
        c.nx[:] = self.nx
        if check:
            self.workspace_bytes(batch, cams, c)
        return c

    def workspace_bytes(self, batch, cams, cfg=None):
        n = C.c_size_t(0)
        lib = M.load()
        M.check(lib.ddp_lss_workspace(C.byref(cfg or self.cfg(batch, cams)), C.byref(n)), lib)
        return int(n.value)

    def use_workspace(self, ws):
        """run in a caller's uint8 device buffer (256-byte aligned, at least ``workspace_bytes`` of every later call)"""
        if not torch.is_tensor(ws) or not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous():
            raise ValueError('the workspace must be a contiguous uint8 device tensor')
        if ws.data_ptr() % M.WS_ALIGN:
            raise ValueError(f'the workspace must be {M.WS_ALIGN}-byte aligned')
        self._ws, self._ws_given, self._shape = ws, True, None
        return self

    def _workspace(self, batch, cams, dev):
        need = self.workspace_bytes(batch, cams)
        if self._ws_given:
            if self._ws.numel() < need or self._ws.device != dev:
                raise ValueError(f'the given workspace holds {self._ws.numel()} bytes on {self._ws.device}, the call needs {need} on {dev}')
        elif self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws

    def plan(self, cam, extra):
        """``cam`` (B, N, 24), ``extra`` (B, 12) device fp32 (``pack_cameras``): the rank of every frustum point and the
        per-cell lists, into the workspace"""
        if not torch.is_tensor(cam) or cam.dim() != 3 or cam.shape[2] != 24:
            raise ValueError('cam must be a (B, N, 24) tensor')
        B, N = int(cam.shape[0]), int(cam.shape[1])
        cam, extra = _dev_f32(cam, 'cam'), _dev_f32(extra, 'extra', (B, 12))
        ws = self._workspace(B, N, cam.device)
        lib = M.load()
        M.check(lib.ddp_lss_plan(C.byref(self.cfg(B, N)), cam.data_ptr(), extra.data_ptr(), ws.data_ptr(), _stream(cam.device)), lib)
        self._shape = (B, N)
        return self

    def plan_from_ranks(self, ranks):
        """the same plan from a (B, N, D, fH, fW) device int32 rank table (-1: dropped)"""
        if not torch.is_tensor(ranks) or not ranks.is_cuda:
            raise ValueError('ranks must be a device tensor: ddp_amd.lss has no CPU path')
        if ranks.dtype != torch.int32 or ranks.dim() != 5 or tuple(ranks.shape[2:]) != (self.D,) + self.feature_size:
            raise ValueError(f'ranks must be int32 of shape (B, N, {self.D}, {self.feature_size[0]}, {self.feature_size[1]})')
        B, N = int(ranks.shape[0]), int(ranks.shape[1])
        ranks = ranks.contiguous()
        ws = self._workspace(B, N, ranks.device)
        lib = M.load()
        M.check(lib.ddp_lss_plan_from_ranks(C.byref(self.cfg(B, N)), ranks.data_ptr(), ws.data_ptr(), _stream(ranks.device)), lib)
        self._shape = (B, N)
        return self

    def _planned(self):
        if self._shape is None:
            raise RuntimeError('no plan in the workspace: call plan() or plan_from_ranks() first')
        return self._shape

    def ranks(self):
        """the plan's rank table: a (B, N, D, fH, fW) int32 view of the workspace"""
        B, N = self._planned()
        lib = M.load()
        p = C.c_void_p(0)
        M.check(lib.ddp_lss_ranks(C.byref(self.cfg(B, N)), self._ws.data_ptr(), C.byref(p)), lib)
        off = p.value - self._ws.data_ptr()
        n = B * N * self.D * self.feature_size[0] * self.feature_size[1]
        return self._ws[off:off + 4 * n].view(torch.int32).view(B, N, self.D, *self.feature_size)

    def pool(self, depthnet_out, out=None):
        """``depthnet_out`` (B * N, D + C, fH, fW) device fp32, as the 1 x 1 convolution emits it -> (B, nz * C, nx0, nx1) fp32,
        channel z * C + c; every element is written (``out``: a caller's contiguous buffer of that shape)"""
        B, N = self._planned()
        x = _dev_f32(depthnet_out, 'depthnet_out', (B * N, self.D + self.C) + self.feature_size)
        shape = (B, self.nx[2] * self.C, self.nx[0], self.nx[1])
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=x.device)
        elif not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous float32 device tensor of shape {shape}')
        lib = M.load()
        M.check(lib.ddp_lss_pool(C.byref(self.cfg(B, N)), x.data_ptr(), self._ws.data_ptr(), out.data_ptr(), _stream(x.device)), lib)
        return out
