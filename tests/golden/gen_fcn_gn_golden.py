#!/usr/bin/env python
"""Golden vectors of FCNHeadWithTime with GroupNorm(32) FROM THE REFERENCE CLASS ITSELF: the head alone and the reference's
ddim_sample / ddpm_sample driving it.

Run by hand in the build container (needs the reference tree, see ``ref_shim``):

    python tests/golden/gen_fcn_gn_golden.py

The reference head is built with ``norm_cfg=dict(type='GN', num_groups=32)``, loaded with the seeded synthetic weights of
``ddp_amd.utils.synthetic`` (``make_fcn_state_dict(..., norm='gn')``) and fed the seeded inputs, exactly as ``gen_golden.py::gen_fcn``
and ``gen_loopfcn`` do for the BatchNorm twins (whose helpers are used here).  Only data is written: per case one
``tests/golden/fcn_gn/<case>.npz`` with the config, the input fingerprints and the reference outputs.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as G  # noqa: E402
from ddp_amd.utils import synthetic  # noqa: E402

GN = dict(type='GN', num_groups=32)
# a directory of their own: golden_util.case_names('fcn') / ('loopfcn') list tests/golden/*.npz by prefix for the BatchNorm loaders
OUT_DIR = os.path.join(HERE, 'fcn_gn')


def save(name, cfg, arrays):
    import json
    import numpy as np
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name + '.npz')
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    np.savez_compressed(path, config=np.array(json.dumps(cfg)), **arrays)
    print(f'wrote {path}  ({os.path.getsize(path) / 1e6:.2f} MB)')

FCN_GN_CASES = [
    dict(name='fcn_gn_2conv', num_convs=2, num_classes=19, with_norm=True, norm='gn', concat_input=True, dilation=1, maps=2, h=12, w=20,
         seed=60, with_time=True),
    dict(name='fcn_gn_dil2_notime', num_convs=2, num_classes=19, with_norm=True, norm='gn', concat_input=False, dilation=2, maps=1, h=10,
         w=14, seed=62, with_time=False),
]

LOOPFCN_GN_CASES = [
    dict(name='loopfcn_gn_k3', h=11, w=15, num_classes=19, timesteps=3, randsteps=1, bit_scale=0.01, accumulation=True,
         diffusion='ddim', num_convs=2, with_norm=True, norm='gn', concat_input=False, dilation=1, seed=70),
    dict(name='loopfcn_gn_ddpm_r2', h=8, w=13, num_classes=19, timesteps=3, randsteps=2, bit_scale=0.01, accumulation=True,
         diffusion='ddpm', num_convs=2, with_norm=True, norm='gn', concat_input=False, dilation=1, seed=71),
]


def _ref_head(case):
    from mmseg.models.decode_heads import FCNHeadWithTime
    return FCNHeadWithTime(num_convs=case['num_convs'], kernel_size=3, concat_input=case['concat_input'], dilation=case['dilation'],
                           in_channels=256, channels=256, num_classes=case['num_classes'], in_index=0, dropout_ratio=0.1,
                           norm_cfg=dict(GN), align_corners=False).eval()


def gen_fcn_gn():
    import ref_shim
    ref_shim.import_seg()
    for case in FCN_GN_CASES:
        head = _ref_head(case)
        sd = synthetic.make_fcn_state_dict(case['num_convs'], case['num_classes'], True, case['concat_input'], case['seed'], norm='gn')
        head.load_state_dict(sd, strict=True)
        feat, temb = synthetic.make_fcn_inputs(case['maps'], case['h'], case['w'], case['seed'])
        times = temb.expand(case['maps'], 1024) if case['with_time'] else None
        with torch.no_grad():
            out = head([feat], times)
        save(case['name'], dict(task='fcn_gn', **case), dict(out=out, feat_fp=G.fingerprint(feat), weights_fp=synthetic.checksum(sd)))


def gen_loopfcn_gn():
    """as gen_golden.py::gen_loopfcn: the segmentor of the ADE config with its decode head replaced by the reference FCN head"""
    import ref_shim
    build_segmentor, Config, revert = ref_shim.import_seg()
    cfg_path = os.path.join(ref_shim.REF, 'segmentation/configs/ade/ddp_swin_t_2x8_512x512_160k_ade20k.py')
    for case in LOOPFCN_GN_CASES:
        cfg = Config.fromfile(cfg_path)
        m = cfg.model
        m.backbone.init_cfg = None
        m.train_cfg = None
        m.timesteps, m.randsteps, m.bit_scale = case['timesteps'], case['randsteps'], case['bit_scale']
        m.accumulation, m.diffusion = case['accumulation'], case['diffusion']
        m.decode_head.num_classes = case['num_classes']
        m.auxiliary_head.num_classes = case['num_classes']
        model = revert(build_segmentor(m)).eval()
        model.decode_head = _ref_head(case)
        model.decode_head.in_channels = [256]
        sd = synthetic.make_fcn_segmentor_state_dict(case['num_convs'], case['num_classes'], True, case['concat_input'],
                                                     case['seed'] + 100, norm='gn')
        G.load_hot_path(model, sd)
        x, noise = synthetic.make_inputs(1, case['h'], case['w'], case['randsteps'], 256, 256, seed=case['seed'])
        step_noise = None
        if case['diffusion'] == 'ddpm':
            g = torch.Generator().manual_seed(case['seed'] + 7)
            step_noise = torch.randn((case['timesteps'], case['randsteps'], 256, case['h'], case['w']), generator=g)
        logits = []
        G.wrap_forward(model.decode_head, logits)
        with torch.no_grad(), G.RandnPatch(noise[0], None if step_noise is None else list(step_noise)):
            out = model.ddim_sample(x, None) if case['diffusion'] == 'ddim' else model.ddpm_sample(x, None)
        save(case['name'], dict(task='loopfcn_gn', **case),
               dict(out=out, logits_steps=torch.stack(logits), x_fp=G.fingerprint(x), noise_fp=G.fingerprint(noise),
                    weights_fp=synthetic.checksum(sd)))


if __name__ == '__main__':
    gen_fcn_gn()
    gen_loopfcn_gn()
