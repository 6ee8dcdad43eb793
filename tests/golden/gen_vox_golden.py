"""Fixtures of the device-side hard voxelisation: the cases ``vox_cases.FIXTURES`` and ``vox_edge_cases.FIXTURES`` run through the
REFERENCE's own code on the CPU.

    python tests/golden/gen_vox_golden.py [out_dir [case ...]]         (by hand, where the reference tree is present)

What is the reference's: ``hard_voxelize_cpu`` (bev/mmdet3d/ops/voxel/src/voxelization_cpu.cpp, compiled here by
``torch.utils.cpp_extension.load`` together with a binding of a few lines that this file writes, into a directory OUTSIDE the
repository), the ``Voxelization`` module and its autograd function (bev/mmdet3d/ops/voxel/voxelize.py, loaded by file path), and
``BEVFusion.voxelize`` (bev/mmdet3d/models/fusion_models/bevfusion.py, loaded by file path and called on an instance made with
``object.__new__`` whose lidar encoder holds that module).  What is this file's: stubs for what those files import - ``mmcv.runner``'s
two decorators as the identity, empty builders and registries, and ``voxel_layer.hard_voxelize`` forwarding to the compiled function.

Every fixture grid has grid_x == grid_z: the reference's CPU function allocates its cell table {grid_z, grid_y, grid_x} and indexes
it [x][y][z] (voxelization_cpu.cpp:75,129-130), so any other grid reads and writes out of bounds.

Writes tests/golden/vox/vox_<case>.npz: the points of each sample, per sample the reference's triple (``voxels<b>``, ``coors<b>``,
``num<b>``), the batched ``feats`` (means), ``feats_raw``, ``coords``, ``sizes``, and ``config``, one JSON string.  Each file stays below
128 KiB.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'vox')
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get('DDP_REFERENCE_ROOT', '/root/reference')
VOXEL = os.path.join(REF, 'bev', 'mmdet3d', 'ops', 'voxel')

import vox_cases as VC  # noqa: E402
import vox_edge_cases as VE  # noqa: E402

BINDING = '''#include <torch/extension.h>
#include <vector>
namespace voxelization {
int hard_voxelize_cpu(const at::Tensor& points, at::Tensor& voxels, at::Tensor& coors, at::Tensor& num_points_per_voxel,
                      const std::vector<float> voxel_size, const std::vector<float> coors_range, const int max_points,
                      const int max_voxels, const int NDim);
}
PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) { m.def("hard_voxelize_cpu", &voxelization::hard_voxelize_cpu); }
'''


def compile_reference():
    from torch.utils.cpp_extension import load
    work = os.path.join(tempfile.gettempdir(), 'ddp_vox_reference_build')
    os.makedirs(work, exist_ok=True)
    binding = os.path.join(work, 'binding.cpp')
    with open(binding, 'w') as f:
        f.write(BINDING)
    return load(name='ddp_vox_reference', sources=[os.path.join(VOXEL, 'src', 'voxelization_cpu.cpp'), binding], build_directory=work,
                extra_cflags=['-O1'], verbose=False)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    """-> the reference's ``Voxelization`` and ``BEVFusion`` classes"""
    ext = compile_reference()

    def pkg(name, **members):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(members)
        sys.modules[name] = m
        return m

    def hard_voxelize(points, voxels, coors, num, voxel_size, coors_range, max_points, max_voxels, ndim, deterministic):
        return ext.hard_voxelize_cpu(points, voxels, coors, num, [float(v) for v in voxel_size], [float(v) for v in coors_range],
                                     int(max_points), int(max_voxels), int(ndim))

    def refuse(*a, **k):
        raise NotImplementedError('not part of these fixtures')

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    identity = lambda *a, **k: (lambda fn: fn)
    pkg('mmcv')
    pkg('mmcv.runner', auto_fp16=identity, force_fp32=identity)
    pkg('mmdet3d')
    pkg('mmdet3d.ops.voxel')
    pkg('mmdet3d.ops.voxel.voxel_layer', hard_voxelize=hard_voxelize, dynamic_voxelize=refuse)
    voxelize = _load('mmdet3d.ops.voxel.voxelize', os.path.join(VOXEL, 'voxelize.py'))
    pkg('mmdet3d.ops', Voxelization=voxelize.Voxelization, DynamicScatter=refuse)
    pkg('mmdet3d.models', FUSIONMODELS=_Registry())
    pkg('mmdet3d.models.builder', **{n: refuse for n in ('build_backbone', 'build_fuser', 'build_head', 'build_neck', 'build_vtransform')})
    pkg('mmdet3d.models.fusion_models')
    pkg('mmdet3d.models.fusion_models.base', Base3DFusionModel=torch.nn.Module)
    fusion = _load('mmdet3d.models.fusion_models.bevfusion', os.path.join(REF, 'bev', 'mmdet3d', 'models', 'fusion_models', 'bevfusion.py'))
    return voxelize.Voxelization, fusion.BEVFusion


def gen(names=None, out=OUT):
    """``names``: the cases to run (default: every committed fixture); ``out``: where the files go"""
    torch.set_num_threads(1)
    Voxelization, BEVFusion = load_reference()
    os.makedirs(out, exist_ok=True)
    sizes = {}
    for name in VC.FIXTURES + VE.FIXTURES if names is None else names:
        c = VC.case(name) if name in VC.NAMES else VE.case(name)
        assert c['grid'][0] == c['grid'][2], name
        module = Voxelization(c['voxel_size'], c['range'], c['T'], (c['max_voxels'] + 1000, c['max_voxels'])).eval()
        assert [int(v) for v in module.grid_size] == c['grid']
        points = [torch.from_numpy(p[:, :c['F']].copy()) for p in c['points']]
        arrays = dict(config=np.asarray(VC.config_of(c)))
        for b, p in enumerate(points):
            voxels, coors, num = module(p)
            arrays.update({f'points{b}': c['points'][b], f'voxels{b}': voxels.numpy(), f'coors{b}': coors.numpy(), f'num{b}': num.numpy()})
        model = object.__new__(BEVFusion)
        model.encoders = {'lidar': {'voxelize': module}}
        for key, reduce in (('feats', True), ('feats_raw', False)):
            model.voxelize_reduce = reduce
            feats, coords, sz = BEVFusion.voxelize(model, points)
            arrays[key] = feats.numpy()
        arrays.update(coords=coords.numpy(), sizes=sz.numpy() if torch.is_tensor(sz) else np.zeros(0, np.int32))
        path = os.path.join(out, f'vox_{name}.npz')
        np.savez_compressed(path, **arrays)
        sizes[os.path.basename(path)] = os.path.getsize(path)
        assert sizes[os.path.basename(path)] <= 128 * 1024, (path, sizes)
    return sizes


if __name__ == '__main__':
    for k, v in gen(sys.argv[2:] or None, *sys.argv[1:2]).items():
        print(k, v, 'bytes')
