"""Fixtures of the device-side LSS lift and pool: the cases of tests/lss_cases.py run through the REFERENCE's own ``LSSTransform``
(bev/mmdet3d/models/vtransforms/base.py and lss.py, loaded by file path) on the CPU.

    python tests/golden/gen_lss_golden.py          (by hand, where the reference tree is present)

Three stubs of this file stand in for what those two files import: ``mmcv.runner.force_fp32`` as the identity decorator, a registry
for ``mmdet3d.models.builder.VTRANSFORMS``, and ``mmdet3d.ops.bev_pool`` - whose CUDA binary the reference tree does not hold - as
an ``index_add_`` into (B, nz, nx0, nx1, C) followed by ``permute(0, 4, 1, 2, 3)``.  So THE POOLED SUM IS THE STUB'S; everything
else - the frustum, the geometry, the cell indices, the kept mask, the softmax, the lift, the z collapse, ``downsample`` - is the
reference's.

Writes, per case, tests/golden/lss/lss_<case>.npz (the inputs, the state dict, the fp32 geometry, the kept mask with the ranks the
reference's indices give, the output with ``downsample=1``) and lss_<case>_ds2.npz (the state dict and the output of the
``downsample=2`` module, which shares ``depthnet``; not for a case with nz > 1 - ``odd``, ``c129``, ``c256`` -, whose nz * C
channels the reference's downsample stack cannot take).  The synthetic cases of ``lss_cases.SYNTH`` have no geometry and no fixture.
Arrays only.  Parameters are rounded to multiples of 2^-8 so that the files compress; the ``long`` case has the points of ``cfg``
and does not repeat its geometry.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'lss')          # a directory of its own: the sampler fixtures of tests/golden/*.npz are listed by a glob
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get('DDP_REFERENCE_ROOT', '/root/reference')
VT = os.path.join(REF, 'bev', 'mmdet3d', 'models', 'vtransforms')

import lss_cases as LC  # noqa: E402

RECORD = {}


def _bev_pool_stub(x, geom_feats, B, D, H, W):
    geom_feats = geom_feats.long()
    flat = ((geom_feats[:, 3] * int(D) + geom_feats[:, 2]) * int(H) + geom_feats[:, 0]) * int(W) + geom_feats[:, 1]
    RECORD['flat'] = flat.clone()
    RECORD['x'] = x.clone()
    out = torch.zeros(int(B) * int(D) * int(H) * int(W), x.shape[1], dtype=x.dtype)
    out.index_add_(0, flat, x)
    return out.view(int(B), int(D), int(H), int(W), x.shape[1]).permute(0, 4, 1, 2, 3)


class _Registry:
    def register_module(self, *a, **k):
        return lambda cls: cls


def load_reference():
    def pkg(name):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        return m
    for name in ('mmcv', 'mmdet3d', 'mmdet3d.models', 'mmdet3d.models.vtransforms'):
        pkg(name)
    runner = types.ModuleType('mmcv.runner')
    runner.force_fp32 = lambda *a, **k: (lambda fn: fn)
    sys.modules['mmcv.runner'] = runner
    ops = types.ModuleType('mmdet3d.ops')
    ops.bev_pool = _bev_pool_stub
    sys.modules['mmdet3d.ops'] = ops
    builder = types.ModuleType('mmdet3d.models.builder')
    builder.VTRANSFORMS = _Registry()
    sys.modules['mmdet3d.models.builder'] = builder
    mods = {}
    for stem in ('base', 'lss'):
        name = 'mmdet3d.models.vtransforms.' + stem
        spec = importlib.util.spec_from_file_location(name, os.path.join(VT, stem + '.py'))
        mods[stem] = importlib.util.module_from_spec(spec)
        sys.modules[name] = mods[stem]
        spec.loader.exec_module(mods[stem])
    return mods['lss'].LSSTransform


def _settle(module, seed):
    """deterministic, compressible parameters: multiples of 2^-8; non-trivial BatchNorm statistics"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if k in ('dx', 'bx', 'nx', 'frustum') or not v.is_floating_point():
                continue
            if k.endswith('running_var'):
                v.copy_(0.5 + torch.randint(0, 256, v.shape, generator=g) / 256.0)
            elif k.endswith('running_mean'):
                v.copy_(torch.randint(-64, 64, v.shape, generator=g) / 256.0)
            else:
                v.copy_(torch.round(v * 256.0) / 256.0)
    return module.eval()


def gen():
    LSSTransform = load_reference()
    os.makedirs(OUT, exist_ok=True)
    sizes = {}
    for i, name in enumerate(LC.NAMES):
        c = LC.case(name)
        torch.manual_seed(100 + i)
        m1 = _settle(LSSTransform(downsample=1, **c['kwargs']), 7 + i)
        with_ds2 = c['nx'][2] == 1          # the reference's downsample stack takes C channels: it cannot follow nz > 1
        if with_ds2:
            m2 = LSSTransform(downsample=2, **c['kwargs'])
            m2.depthnet.load_state_dict(m1.depthnet.state_dict())
            _settle(m2, 70 + i)
        args = LC.forward_args(c)
        geoms = {}
        orig = m1.get_geometry
        m1.get_geometry = lambda *a, **k: geoms.setdefault('g', orig(*a, **k))
        with torch.no_grad():
            out1 = m1(*args)
            out2 = m2(*args) if with_ds2 else None
            geom = geoms['g']
            # the kept mask: the reference's own bev_pool once more, on a volume that carries the point index (exact in fp32)
            assert c['P'] < 2 ** 24
            idx = torch.arange(c['P'], dtype=torch.float32).view(c['B'], c['N'], c['D'], c['fH'], c['fW'], 1)
            m1.bev_pool(geom, idx)
        kept_idx = RECORD['x'][:, 0].long().numpy()
        kept = np.zeros(c['P'], dtype=bool)
        kept[kept_idx] = True
        ranks = np.full(c['P'], -1, dtype=np.int32)
        ranks[kept_idx] = RECORD['flat'].numpy().astype(np.int32)
        main = dict(img=c['img'].numpy(), camera2lidar=c['camera2lidar'].numpy(), camera_intrinsics=c['camera_intrinsics'].numpy(),
                    img_aug_matrix=c['img_aug_matrix'].numpy(), lidar_aug_matrix=c['lidar_aug_matrix'].numpy(), kept=kept, ranks=ranks,
                    out=out1.numpy())
        if 'same_points_as' not in LC.CASES[name]:
            main['geom'] = geom.reshape(-1, 3).numpy()
        for k, v in m1.state_dict().items():
            main['sd/' + k] = v.numpy()
        files = [('', main)]
        if with_ds2:
            ds2 = dict(out=out2.numpy())
            for k, v in m2.state_dict().items():
                ds2['sd/' + k] = v.numpy()
            files.append(('_ds2', ds2))
        for suffix, arrays in files:
            path = os.path.join(OUT, f'lss_{name}{suffix}.npz')
            np.savez_compressed(path, **arrays)
            sizes[os.path.basename(path)] = os.path.getsize(path)
    return sizes


if __name__ == '__main__':
    for k, v in gen().items():
        print(k, v, 'bytes')
