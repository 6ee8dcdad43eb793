"""``LSSTransform`` of the camera-only BEV configuration (bev/mmdet3d/models/vtransforms/lss.py + base.py ``BaseTransform``) with the
lift and pool on the device (ddp_amd/lss.py, libddp_lss.so).  Same constructor arguments, members and state-dict keys as the
reference class, so a checkpoint loads with ``strict=True``; ``depthnet`` and ``downsample`` stay torch modules.  Inference only."""
import torch
from torch import nn

from .. import lss as _lss
from ..registry import VTRANSFORMS


@VTRANSFORMS.register_module(name='LSSTransform')
class LSSTransform(nn.Module):
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
        self.depthnet = nn.Conv2d(in_channels, self.D + self.C, 1)
        if downsample > 1:
            assert downsample == 2, downsample
            self.downsample = nn.Sequential(
                nn.Conv2d(out_channels, out_channels, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True),
                nn.Conv2d(out_channels, out_channels, 3, stride=downsample, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True),
                nn.Conv2d(out_channels, out_channels, 3, padding=1, bias=False), nn.BatchNorm2d(out_channels), nn.ReLU(True))
        else:
            self.downsample = nn.Identity()
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

    @torch.no_grad()
    def forward(self, img, points, camera2ego, lidar2ego, lidar2camera, lidar2image, camera_intrinsics, camera2lidar, img_aug_matrix,
                lidar_aug_matrix, metas, **kwargs):
        if not img.is_cuda:
            raise ValueError('LSSTransform runs on the device: ddp_amd.lss has no CPU path')
        B, N, C, fH, fW = img.shape
        x = self.depthnet(img.float().view(B * N, C, fH, fW))
        cam, extra = _lss.pack_cameras(camera2lidar[..., :3, :3].float(), camera2lidar[..., :3, 3].float(),
                                       camera_intrinsics[..., :3, :3].float(), img_aug_matrix[..., :3, :3].float(),
                                       img_aug_matrix[..., :3, 3].float(), lidar_aug_matrix[..., :3, :3].float(),
                                       lidar_aug_matrix[..., :3, 3].float())
        x = self.pooler.plan(cam, extra).pool(x)
        return self.downsample(x)
