"""``Voxelization`` of the camera + lidar BEV configuration's lidar branch (bev/mmdet3d/ops/voxel/voxelize.py) with the hard
voxelisation on the device (ddp_amd/vox.py, libddp_vox.so).  Same constructor arguments, members and ``__repr__`` as the reference
class; ``forward`` returns its triple.  The result is the reference's deterministic one whatever ``deterministic`` says.  Not built,
refused by message: the dynamic path (``max_num_points == -1`` or a ``max_voxels`` of -1), fp16 points, any backward."""
import torch
from torch import nn
from torch.nn.modules.utils import _pair

from .. import vox as _vox


class Voxelization(nn.Module):
    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000, deterministic=True):
        super().__init__()
        self.voxel_size = voxel_size
        self.point_cloud_range = point_cloud_range
        self.max_num_points = max_num_points
        self.max_voxels = max_voxels if isinstance(max_voxels, tuple) else _pair(max_voxels)
        self.deterministic = deterministic          # accepted and ignored: the result is always the deterministic one
        grid_size = _vox.grid_of(voxel_size, point_cloud_range)
        self.grid_size = grid_size
        # the reference keeps [x-len, y-len, 1] (voxelize.py:115-119)
        self.pcd_shape = [*grid_size[:2], 1]
        if max_num_points == -1 or -1 in self.max_voxels:
            raise NotImplementedError('max_num_points == -1 or max_voxels == -1 is the dynamic path (DynamicScatter): not built')
        self._engines = {}                          # one HardVoxelizer per voxel cap in use: (training, testing)

    def engine(self, max_voxels=None):
        """the HardVoxelizer of a voxel cap (default: the cap of the module's mode)"""
        cap = int(self.max_voxels[0 if self.training else 1] if max_voxels is None else max_voxels)
        if cap not in self._engines:
            self._engines[cap] = _vox.HardVoxelizer(self.voxel_size, self.point_cloud_range, self.max_num_points, cap)
        return self._engines[cap]

    @torch.no_grad()
    def forward(self, input):
        """``input``: (P, F) device fp32 points -> voxels (M, max_num_points, F), coors (M, 3) int32 x y z, num_points (M) int32, tensors
        of their own (not views of the engine's buffers)"""
        return tuple(t.clone() for t in self.engine().voxelize(input))

    def __repr__(self):
        shown = ('voxel_size', 'point_cloud_range', 'max_num_points', 'max_voxels', 'deterministic')
        return f'{type(self).__name__}(' + ', '.join(f'{k}={getattr(self, k)}' for k in shown) + ')'
