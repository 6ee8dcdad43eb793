"""Fixtures of the device-side front of ``DepthLSSTransform``: the cases of tests/dlss_cases.py run through the REFERENCE's own
``DepthLSSTransform`` and ``BaseDepthTransform`` (bev/mmdet3d/models/vtransforms/depth_lss.py and base.py, loaded by file path) on
the CPU, under ``torch.set_num_threads(1)`` - where the reference's indexed assignment is "the last point in point order wins" - and
with the BLAS in its reproducible mode (``MKL_CBWR=COMPATIBLE``, set below), so that the recorded numbers are no CPU's own.

    python tests/golden/gen_dlss_golden.py          (by hand, where the reference tree is present)

The three stubs of gen_lss_golden.py stand in for what those files import: ``mmcv.runner.force_fp32`` as the identity decorator, a
registry for ``mmdet3d.models.builder.VTRANSFORMS``, and ``mmdet3d.ops.bev_pool`` - whose CUDA binary the reference tree does not
hold - as an ``index_add_`` into (B, nz, nx0, nx1, C).  So THE POOLED SUM IS THE STUB'S; everything else - the projection, the depth
image, ``dtransform``, ``depthnet``, the geometry, the softmax, the lift, ``downsample`` - is the reference's.

Writes, per case but ``wide``, tests/golden/dlss/dlss_<case>.npz: the inputs (points, features, matrices), the state dict (``sd/``),
the fp32 ``inverse(lidar_aug[:3, :3])`` of base.py:251, the depth image, the ``dtransform[0:6]`` output, the output with
``downsample=1`` and, where nz = 1, the ``downsample.*`` entries (``sd2/``) and the output (``out2``) of a ``downsample=2`` module that
shares every other parameter.  Arrays only.  Parameters are rounded to multiples of 2^-8 so that the files compress.
"""
import importlib.util
import os
import sys

# The reference's three ``matmul`` calls go to the BLAS, whose summation order and use of fused multiply-add depend on the CPU it finds.
# Its conditional-numerical-reproducibility mode gives, on every CPU, the product summed left to right with one rounding per operation
# - the restatement of tests/dlss_cases.py and the convention of the device kernel.  Set before torch loads the BLAS.
os.environ['MKL_CBWR'] = 'COMPATIBLE'

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'dlss')
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dlss_cases as DC  # noqa: E402
import gen_lss_golden as G  # noqa: E402


def load_reference():
    G.load_reference()                       # the stubs, base.py and lss.py
    name = 'mmdet3d.models.vtransforms.depth_lss'
    spec = importlib.util.spec_from_file_location(name, os.path.join(G.VT, 'depth_lss.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod.DepthLSSTransform


def gen():
    torch.set_num_threads(1)
    DepthLSSTransform = load_reference()
    os.makedirs(OUT, exist_ok=True)
    sizes = {}
    for i, name in enumerate(DC.FIXTURES):
        c = DC.case(name)
        torch.manual_seed(300 + i)
        m1 = G._settle(DepthLSSTransform(downsample=1, **c['kwargs']), 17 + i)
        seen = {}
        m1.dtransform.register_forward_pre_hook(lambda mod, inp: seen.setdefault('depth', inp[0].detach().clone()))
        m1.dtransform[5].register_forward_hook(lambda mod, inp, out: seen.setdefault('stem', out.detach().clone()))
        with torch.no_grad():
            out1 = m1(*DC.forward_args(c))
        arrays = dict(img=c['img'].numpy(), lidar2image=c['lidar2image'].numpy(), camera2lidar=c['camera2lidar'].numpy(),
                      camera_intrinsics=c['camera_intrinsics'].numpy(), img_aug_matrix=c['img_aug_matrix'].numpy(),
                      lidar_aug_matrix=c['lidar_aug_matrix'].numpy(), seed=np.int64(c['seed']),
                      lidar_aug_inverse=torch.inverse(c['lidar_aug_matrix'][:, :3, :3]).numpy(),      # base.py:251, the same call
                      depth=seen['depth'].view(c['B'], c['N'], 1, c['iH'], c['iW']).numpy(), stem=seen['stem'].numpy(), out=out1.numpy())
        for b, p in enumerate(c['points']):
            arrays[f'points{b}'] = p.numpy()
        for k, v in m1.state_dict().items():
            arrays['sd/' + k] = v.numpy()
        if c['nx'][2] == 1:                  # the reference's downsample stack takes C channels: it cannot follow nz > 1
            m2 = DepthLSSTransform(downsample=2, **c['kwargs'])
            m2.load_state_dict(m1.state_dict(), strict=False)
            G._settle(m2.downsample, 170 + i)
            m2.eval()
            with torch.no_grad():
                arrays['out2'] = m2(*DC.forward_args(c)).numpy()
            for k, v in m2.downsample.state_dict().items():
                arrays['sd2/downsample.' + k] = v.numpy()
        path = os.path.join(OUT, f'dlss_{name}.npz')
        np.savez_compressed(path, **arrays)
        sizes[os.path.basename(path)] = os.path.getsize(path)
    return sizes


if __name__ == '__main__':
    for k, v in gen().items():
        print(k, v, 'bytes')
