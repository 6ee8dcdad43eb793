"""``DepthLSSTransform`` of the camera + lidar BEV configuration (bev/mmdet3d/models/vtransforms/depth_lss.py + base.py
``BaseDepthTransform``) with the lidar depth image, the ``dtransform`` stem and the lift and pool on the device (ddp_amd/dlss.py,
libddp_dlss.so; ddp_amd/lss.py, libddp_lss.so).  Same constructor arguments, members and state-dict keys as the reference class, so a
checkpoint loads with ``strict=True``; the third ``dtransform`` convolution, ``depthnet`` and ``downsample`` stay torch modules.
Inference only, eval-mode BatchNorm: a module in training mode raises."""
import torch
from torch import nn

from .. import dlss as _dlss
from .. import lss as _lss
from ..registry import VTRANSFORMS


@VTRANSFORMS.register_module(name='DepthLSSTransform')
class DepthLSSTransform(nn.Module):
    """The one deliberate difference to the reference: ``forward`` does NOT modify the caller's ``points``.  The reference subtracts the
    lidar augmentation's translation from ``points[b][:, :3]`` in place (base.py:250); here the points are only read.

    Where two points of one camera fall on the same pixel, the one with the larger point index wins - what the reference's indexed
    assignment does on one CPU thread and leaves undefined on a GPU.  The stored depth is the z clamped to [1e-5, 1e5], as there."""

    def __init__(self, in_channels, out_channels, image_size, feature_size, xbound, ybound, zbound, dbound, downsample=1):
        super().__init__()
        self.in_channels = in_channels
        self.image_size = image_size
        self.feature_size = feature_size
        self.xbound = xbound
        self.ybound = ybound
        self.zbound = zbound
        self.dbound = dbound
        dx, bx, nx = _lss.grid_of(xbound, ybound, zbound)
        self.dx = nn.Parameter(dx, requires_grad=False)
        self.bx = nn.Parameter(bx, requires_grad=False)
        self.nx = nn.Parameter(nx, requires_grad=False)
        self.C = out_channels
        self.frustum = self.create_frustum()
        self.D = self.frustum.shape[0]
        self.fp16_enabled = False
        self.dtransform = nn.Sequential(
            nn.Conv2d(1, 8, 1), nn.BatchNorm2d(8), nn.ReLU(True),
            nn.Conv2d(8, 32, 5, stride=4, padding=2), nn.BatchNorm2d(32), nn.ReLU(True),
            nn.Conv2d(32, 64, 5, stride=2, padding=2), nn.BatchNorm2d(64), nn.ReLU(True))
        self.depthnet = nn.Sequential(
            nn.Conv2d(in_channels + 64, in_channels, 3, padding=1), nn.BatchNorm2d(in_channels), nn.ReLU(True),
            nn.Conv2d(in_channels, in_channels, 3, padding=1), nn.BatchNorm2d(in_channels), nn.ReLU(True),
            nn.Conv2d(in_channels, self.D + self.C, 1))
        if downsample > 1:
            assert downsample == 2, downsample
            self.downsample = nn.Sequential(
                nn.Conv2d(out_channels, out_channels, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True),
                nn.Conv2d(out_channels, out_channels, 3, stride=downsample, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True),
                nn.Conv2d(out_channels, out_channels, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True))
        else:
            self.downsample = nn.Identity()
        self.lidar_depth = _dlss.LidarDepth(image_size)
        self.pooler = _lss.LssPool(image_size, feature_size, xbound, ybound, zbound, dbound, out_channels)

    def create_frustum(self):
        """(D, fH, fW, 3) of (xs[w], ys[h], ds[d]); a state-dict entry of the reference, kept for its checkpoints - the kernel forms
        the same numbers itself"""
        iH, iW = self.image_size
        fH, fW = self.feature_size
        ds = torch.arange(*self.dbound, dtype=torch.float).view(-1, 1, 1).expand(-1, fH, fW)
        D = ds.shape[0]
        xs = torch.linspace(0, iW - 1, fW, dtype=torch.float).view(1, 1, fW).expand(D, fH, fW)
        ys = torch.linspace(0, iH - 1, fH, dtype=torch.float).view(1, fH, 1).expand(D, fH, fW)
        return nn.Parameter(torch.stack((xs, ys, ds), -1), requires_grad=False)

    def depth_image(self, points, lidar2image, img_aug_matrix, lidar_aug_matrix):
        """the (B, N, 1, iH, iW) lidar depth image of base.py:238-279, on the device; ``points`` is left as it is"""
        return self.lidar_depth.project(points, lidar2image, img_aug_matrix, lidar_aug_matrix).scatter()

    @torch.no_grad()
    def forward(self, img, points, sensor2ego, lidar2ego, lidar2camera, lidar2image, cam_intrinsic, camera2lidar, img_aug_matrix,
                lidar_aug_matrix, metas, **kwargs):
        if self.training:
            raise RuntimeError('DepthLSSTransform is inference only (eval-mode BatchNorm, no backward): call .eval()')
        if not torch.is_tensor(img) or not img.is_cuda:
            raise ValueError('DepthLSSTransform runs on the device: ddp_amd.dlss has no CPU path')
        B, N, C, fH, fW = img.shape
        depth = self.depth_image(points, lidar2image, img_aug_matrix, lidar_aug_matrix)
        d = self.lidar_depth.stem(depth, self.dtransform)
        d = self.dtransform[6:](d)
        x = self.depthnet(torch.cat([d, img.float().view(B * N, C, fH, fW)], dim=1))
        cam, extra = _lss.pack_cameras(camera2lidar[..., :3, :3].float(), camera2lidar[..., :3, 3].float(),
                                       cam_intrinsic[..., :3, :3].float(), img_aug_matrix[..., :3, :3].float(),
                                       img_aug_matrix[..., :3, 3].float(), lidar_aug_matrix[..., :3, :3].float(),
                                       lidar_aug_matrix[..., :3, 3].float())
        x = self.pooler.plan(cam, extra).pool(x.contiguous())
        return self.downsample(x)
