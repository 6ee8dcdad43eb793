"""Host layer of libddp_dlss.so (include/ddp_dlss_mi355x.h): what the reference's ``BaseDepthTransform.forward``
(bev/mmdet3d/models/vtransforms/base.py:209-295) and ``DepthLSSTransform.get_cam_feats`` (depth_lss.py) run in front of the lift and
pool, on the device.

  ``pack_lidar``   the (B, 12) / (B * N, 24) matrix tables of one batch: the 3 x 3 inverse of ``lidar_aug`` stays a torch op
  ``LidarDepth``   owns the workspace: ``project`` (``project_packed``) / ``tables`` / ``scatter`` / ``scatter_from_tables`` / ``stem``

There is no CPU fallback: CPU tensors raise.  The caller's points are only read.
"""
import ctypes as C

import torch

from . import _dlss_lib as M
from .evaluation import _stream


def pack_lidar(lidar2image, img_aug_matrix, lidar_aug_matrix):
    """-> lidar (B, 12), cam (B, N, 24) fp32, where the inputs live: inverse(lidar_aug_rot) 9, lidar_aug_trans 3; lidar2image_rot 9,
    lidar2image_trans 3, img_aug_rot 9, img_aug_trans 3 (base.py:245-264)."""
    B, N = int(lidar2image.shape[0]), int(lidar2image.shape[1])
    l2i, aug, laug = lidar2image.float(), img_aug_matrix.float(), lidar_aug_matrix.float()
    lidar = torch.cat([torch.inverse(laug[:, :3, :3]).reshape(B, 9), laug[:, :3, 3].reshape(B, 3)], dim=1).contiguous()
    cam = torch.cat([l2i[..., :3, :3].reshape(B, N, 9), l2i[..., :3, 3].reshape(B, N, 3), aug[..., :3, :3].reshape(B, N, 9),
                     aug[..., :3, 3].reshape(B, N, 3)], dim=2).contiguous()
    return lidar, cam


def stem_size(image_size):
    """the output size of the two stem stages: 1 x 1, then 5 x 5 stride 4 padding 2"""
    return (int(image_size[0]) - 1) // 4 + 1, (int(image_size[1]) - 1) // 4 + 1


def _dev(t, what, dtype=torch.float32, shape=None):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f'{what} must be a device tensor: ddp_amd.dlss has no CPU path')
    if t.dtype != dtype:
        raise ValueError(f'{what} must be {dtype}, got {t.dtype}')
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'{what} must have shape {tuple(shape)}, got {tuple(t.shape)}')
    return t.contiguous()


class LidarDepth:
    """The device depth image of one image size.  ``project`` fixes (B, N, Pmax) and leaves the pixel and depth tables in the workspace
    this object owns; ``scatter`` uses them.  Nothing synchronises."""

    def __init__(self, image_size):
        self.image_size = tuple(int(v) for v in image_size)
        self._shape = None            # (B, N, Pmax) of the tables in the workspace
        self._ws = None
        self._ws_given = False
        self._keep = None             # the tensors the last project() read: alive while a captured graph may replay it
        self._keep_stem = None
        self.workspace_bytes(1, 1, 0)  # refuse an image outside the library's limits here, not at the first call

    def cfg(self, batch, cams, pmax):
        return M.Cfg(int(batch), int(cams), self.image_size[0], self.image_size[1], int(pmax))

    def workspace_bytes(self, batch, cams, pmax):
        n = C.c_size_t(0)
        lib = M.load()
        M.check(lib.ddp_dlss_workspace(C.byref(self.cfg(batch, cams, pmax)), C.byref(n)), lib)
        return int(n.value)

    def use_workspace(self, ws):
        """run in a caller's uint8 device buffer (256-byte aligned, at least ``workspace_bytes`` of every later call)"""
        if not torch.is_tensor(ws) or not ws.is_cuda or ws.dtype != torch.uint8 or not ws.is_contiguous():
            raise ValueError('the workspace must be a contiguous uint8 device tensor')
        if ws.data_ptr() % M.WS_ALIGN:
            raise ValueError(f'the workspace must be {M.WS_ALIGN}-byte aligned')
        self._ws, self._ws_given, self._shape = ws, True, None
        return self

    def _workspace(self, shape, dev):
        need = self.workspace_bytes(*shape)
        if self._ws_given:
            if self._ws.numel() < need or self._ws.device != dev:
                raise ValueError(f'the given workspace holds {self._ws.numel()} bytes on {self._ws.device}, the call needs {need} on {dev}')
        elif self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
            self._shape = None        # a new buffer holds no tables
        return self._ws

    def project(self, points, lidar2image, img_aug_matrix, lidar_aug_matrix, pmax=None):
        """``points``: a list of B (P_b, >= 3) device fp32 tensors (rows x, y, z, ...), read in place and never written;
        ``lidar2image`` and ``img_aug_matrix`` (B, N, 4, 4), ``lidar_aug_matrix`` (B, 4, 4).  ``pmax``: rows the tables reserve per
        sample (default: the largest count)."""
        if not isinstance(points, (list, tuple)) or not points:
            raise ValueError('points must be a non-empty list of (P, >= 3) tensors, one per sample')
        B = len(points)
        if not torch.is_tensor(lidar2image) or lidar2image.dim() != 4 or tuple(lidar2image.shape[2:]) != (4, 4) or lidar2image.shape[0] != B:
            raise ValueError('lidar2image must be a (B, N, 4, 4) tensor with one entry per sample of points')
        N = int(lidar2image.shape[1])
        for what, t, shape in (('lidar2image', lidar2image, (B, N, 4, 4)), ('img_aug_matrix', img_aug_matrix, (B, N, 4, 4)),
                               ('lidar_aug_matrix', lidar_aug_matrix, (B, 4, 4))):
            if not torch.is_tensor(t) or not t.is_cuda:
                raise ValueError(f'{what} must be a device tensor: ddp_amd.dlss has no CPU path')
            if tuple(t.shape) != shape:
                raise ValueError(f'{what} must have shape {shape}, got {tuple(t.shape)}')
        return self.project_packed(points, *pack_lidar(lidar2image, img_aug_matrix, lidar_aug_matrix), pmax=pmax)

    def project_packed(self, points, lidar, cam, pmax=None):
        """the same from the (B, 12) and (B, N, 24) tables of ``pack_lidar``: the library call alone, as a graph captures it"""
        if not isinstance(points, (list, tuple)) or not points:
            raise ValueError('points must be a non-empty list of (P, >= 3) tensors, one per sample')
        B = len(points)
        if not torch.is_tensor(cam) or cam.dim() != 3 or cam.shape[2] != 24 or cam.shape[0] != B:
            raise ValueError('cam must be a (B, N, 24) tensor with one entry per sample of points')
        N = int(cam.shape[1])
        lidar, cam = _dev(lidar, 'lidar', torch.float32, (B, 12)), _dev(cam, 'cam')
        rows, stride = [], None
        for b, p in enumerate(points):
            if not torch.is_tensor(p) or not p.is_cuda:
                raise ValueError(f'points[{b}] must be a device tensor: ddp_amd.dlss has no CPU path')
            if p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] < 3:
                raise ValueError(f'points[{b}] must be float32 of shape (P, >= 3), got {p.dtype} {tuple(p.shape)}')
            if stride is not None and int(p.shape[1]) != stride:
                raise ValueError('every sample of points must have the same number of columns')
            stride = int(p.shape[1])
            rows.append(p.contiguous())   # a copy only of a non-contiguous view; the caller's tensor is never written
        counts = [int(p.shape[0]) for p in rows]
        pmax = max(counts) if pmax is None else int(pmax)
        dev = cam.device
        shape = (B, N, pmax)
        ws = self._workspace(shape, dev)
        lib = M.load()
        ptrs = (C.c_void_p * B)(*[p.data_ptr() if n else None for p, n in zip(rows, counts)])
        cnts = (C.c_int32 * B)(*counts)
        M.check(lib.ddp_dlss_project(C.byref(self.cfg(*shape)), ptrs, cnts, stride, lidar.data_ptr(), cam.data_ptr(), ws.data_ptr(),
                                     _stream(dev)), lib)
        self._shape, self._keep = shape, (rows, lidar, cam)
        return self

    def _projected(self):
        if self._shape is None:
            raise RuntimeError('no tables in the workspace: call project() first')
        return self._shape

    def tables(self):
        """the (B, N, Pmax) pixel (int32, ``row * iW + col`` or -1) and depth (fp32, clamped z) tables: views of the workspace"""
        B, N, pmax = self._projected()
        lib = M.load()
        pp, pd = C.c_void_p(0), C.c_void_p(0)
        M.check(lib.ddp_dlss_pixels(C.byref(self.cfg(B, N, pmax)), self._ws.data_ptr(), C.byref(pp), C.byref(pd)), lib)
        n = B * N * pmax
        base = self._ws.data_ptr()
        view = lambda p, dt: self._ws[p.value - base:p.value - base + 4 * n].view(dt).view(B, N, pmax)
        return view(pp, torch.int32), view(pd, torch.float32)

    def _image(self, B, N, out, dev):
        shape = (B, N, 1) + self.image_size
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=dev)
        if not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous float32 device tensor of shape {shape}')
        return out

    def scatter(self, out=None):
        """the tables of ``project`` -> the (B, N, 1, iH, iW) depth image; every pixel is written (+0.0 where no point falls)"""
        B, N, pmax = self._projected()
        out = self._image(B, N, out, self._ws.device)
        lib = M.load()
        M.check(lib.ddp_dlss_scatter(C.byref(self.cfg(B, N, pmax)), self._ws.data_ptr(), out.data_ptr(), _stream(out.device)), lib)
        return out

    def scatter_from_tables(self, pix, depth, out=None):
        """the same from a caller's (B, N, Pmax) int32 pixel and fp32 depth tables (a pixel outside [0, iH * iW) counts as -1)"""
        if not torch.is_tensor(pix) or pix.dim() != 3:
            raise ValueError('pix must be a (B, N, Pmax) tensor')
        B, N, pmax = (int(v) for v in pix.shape)
        pix = _dev(pix, 'pix', torch.int32)
        depth = _dev(depth, 'depth', torch.float32, (B, N, pmax))
        had, before = self._shape, self._ws
        ws = self._workspace((B, N, pmax), pix.device)
        # the winner image of this call lies behind the projected tables only for the same shape: any other shape overwrites them
        self._shape = had if had == (B, N, pmax) and ws is before else None
        out = self._image(B, N, out, pix.device)
        lib = M.load()
        M.check(lib.ddp_dlss_scatter_from_tables(C.byref(self.cfg(B, N, pmax)), pix.data_ptr(), depth.data_ptr(), ws.data_ptr(),
                                                 out.data_ptr(), _stream(pix.device)), lib)
        return out

    def stem(self, depth, dtransform, out=None):
        """``depth`` (B, N, 1, iH, iW) or (B * N, 1, iH, iW) device fp32, ``dtransform`` the reference's ``nn.Sequential``: its modules
        0, 1, 3 and 4 (conv, BN, conv, BN) hand their parameters to the library as they are -> ``dtransform[0:6](depth)``,
        (B * N, 32, oH, oW), with eval-mode BatchNorm"""
        if not torch.is_tensor(depth) or not depth.is_cuda:
            raise ValueError('depth must be a device tensor: ddp_amd.dlss has no CPU path')
        if depth.dim() not in (4, 5) or tuple(depth.shape[-3:]) != (1,) + self.image_size:
            raise ValueError(f'depth must have shape (B, N, 1, {self.image_size[0]}, {self.image_size[1]})')
        depth = _dev(depth, 'depth')
        BN = int(depth.numel() // (self.image_size[0] * self.image_size[1]))
        conv1, bn1, conv2, bn2 = dtransform[0], dtransform[1], dtransform[3], dtransform[4]
        if bn1.training or bn2.training:
            raise RuntimeError('the stem kernel folds eval-mode BatchNorm: call .eval() on the module')
        if (tuple(conv1.weight.shape) != (M.STEM_MID, 1, 1, 1) or tuple(conv2.weight.shape) != (M.STEM_OUT, M.STEM_MID, 5, 5)
                or conv2.stride != (4, 4) or conv2.padding != (2, 2) or conv1.bias is None or conv2.bias is None):
            raise ValueError('dtransform must start with Conv2d(1, 8, 1), BatchNorm2d(8), ReLU, Conv2d(8, 32, 5, stride=4, padding=2), '
                             'BatchNorm2d(32), ReLU')
        tensors = [conv1.weight, conv1.bias, bn1.weight, bn1.bias, bn1.running_mean, bn1.running_var,
                   conv2.weight, conv2.bias, bn2.weight, bn2.bias, bn2.running_mean, bn2.running_var]
        tensors = [_dev(t.detach(), 'dtransform.' + n[2:]) for t, n in zip(tensors, M.STEM_POINTERS)]
        params = M.StemParams(*[t.data_ptr() for t in tensors], float(bn1.eps), float(bn2.eps))
        # the folded parameters live behind the tables: a shape of the tables, when there is one, keeps them where they are
        shape = self._shape if self._shape is not None and self._shape[0] * self._shape[1] == BN else (1, BN, 0)
        if shape != self._shape:
            self._workspace(shape, depth.device)
            self._shape = None
        ws = self._ws
        oH, oW = stem_size(self.image_size)
        oshape = (BN, M.STEM_OUT, oH, oW)
        if out is None:
            out = torch.empty(oshape, dtype=torch.float32, device=depth.device)
        elif not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != oshape or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous float32 device tensor of shape {oshape}')
        lib = M.load()
        M.check(lib.ddp_dlss_stem(C.byref(self.cfg(*shape)), depth.data_ptr(), C.byref(params), ws.data_ptr(), out.data_ptr(),
                                  _stream(depth.device)), lib)
        self._keep_stem = tensors
        return out
