#!/usr/bin/env python
"""Golden vectors of the binned depth head and of the split depth range, made BY THE REFERENCE ITSELF.

Run by hand in the build container (needs the reference tree, see ``ref_shim``):

    python tests/golden/gen_golden_depth_bins.py

The reference depther is built from the KITTI DDP config with ``decode_head`` overrides (``classify=True``, ``n_bins``,
``bins_strategy``, ``norm_strategy``; or a head depth range that differs from the depther's), loaded with the seeded synthetic
hot-path weights of ``ddp_amd.utils.synthetic`` and run with the seeded start noise in place of its in-method ``torch.randn``
(the helpers of ``gen_golden``).  The fixtures go to ``tests/golden/depth_bins/`` - NOT the top level, whose ``depth_*`` files the
regression-head tests enumerate - one ``<case>.npz`` each: the config, input fingerprints and the reference outputs.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import gen_golden as G  # noqa: E402
from ddp_amd.utils import synthetic  # noqa: E402

OUT = os.path.join(HERE, 'depth_bins')
KITTI = 'depth/configs/ddp_kitti/ddp_swint_1k_w7_kitti_bs2x8_scale01.py'

# sampler cases: depther range (min_depth, max_depth), head overrides in `head`
CASES = [
    dict(name='ud_linear', h=11, w=19, timesteps=3, randsteps=1, bit_scale=0.1, seed=30, min_depth=1e-3, max_depth=80.0,
         head=dict(classify=True, n_bins=256, bins_strategy='UD', norm_strategy='linear')),
    dict(name='ud_softmax_r2', h=11, w=19, timesteps=3, randsteps=2, bit_scale=0.1, seed=31, min_depth=1e-3, max_depth=80.0,
         head=dict(classify=True, n_bins=64, bins_strategy='UD', norm_strategy='softmax')),
    # not a multiple of any tile width; a different step grid
    dict(name='ud_sigmoid_td2', h=11, w=19, timesteps=4, randsteps=1, bit_scale=0.1, seed=32, min_depth=1e-3, max_depth=80.0,
         time_difference=2, head=dict(classify=True, n_bins=100, bins_strategy='UD', norm_strategy='sigmoid')),
    # logspace takes its arguments as base-10 EXPONENTS: [0, 1] gives finite bins 1 .. 10 (KITTI's range would give inf)
    dict(name='sid_softmax', h=11, w=19, timesteps=3, randsteps=1, bit_scale=0.1, seed=33, min_depth=0.0, max_depth=1.0,
         head=dict(classify=True, n_bins=24, bins_strategy='SID', norm_strategy='softmax', min_depth=0.0, max_depth=1.0)),
    # regression heads with their own range: eps = the head's min_depth (relu) / max_depth (scale_up); x0 = the depther's range
    dict(name='range_split', h=11, w=19, timesteps=3, randsteps=1, bit_scale=0.1, seed=34, min_depth=1e-3, max_depth=80.0,
         head=dict(min_depth=0.5, max_depth=10.0)),
    dict(name='range_split_scale_up', h=11, w=19, timesteps=3, randsteps=2, bit_scale=0.1, seed=35, min_depth=1e-3, max_depth=80.0,
         head=dict(min_depth=1e-3, max_depth=10.0, scale_up=True)),
]
# stand-alone head call: decode_head.forward([feat], t) on R maps
HEAD_CASE = dict(name='head_forward', h=11, w=19, R=2, seed=36, t=0.4, min_depth=1e-3, max_depth=80.0,
                 head=dict(classify=True, n_bins=48, bins_strategy='UD', norm_strategy='softmax'))


def save(name, cfg, arrays):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + '.npz')
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    np.savez_compressed(path, config=np.array(json.dumps(cfg)), **arrays)
    print(f'wrote {path}  ({os.path.getsize(path) / 1e6:.3f} MB)')


def build(build_depther, Config, case):
    import ref_shim
    from mmcv.cnn.utils import revert_sync_batchnorm
    cfg = Config.fromfile(os.path.join(ref_shim.REF, KITTI))
    m = cfg.model
    m.backbone.init_cfg = None
    m.train_cfg = None
    m.timesteps = case.get('timesteps', 1)
    m.randsteps = case.get('randsteps', 1)
    m.bit_scale = case.get('bit_scale', 0.1)
    m.min_depth, m.max_depth = case['min_depth'], case['max_depth']
    if 'time_difference' in case:
        m.time_difference = case['time_difference']
    m.decode_head.min_depth, m.decode_head.max_depth = case['min_depth'], case['max_depth']
    for k, v in case['head'].items():
        m.decode_head[k] = v
    model = revert_sync_batchnorm(build_depther(m)).eval()
    sd = synthetic.make_state_dict('depth', 1, 6, 256, seed=case['seed'] + 100, n_bins=case['head'].get('n_bins') if
                                   case['head'].get('classify') else None)
    G.load_hot_path(model, sd)
    return model, sd


def gen_sampler(build_depther, Config, case):
    model, sd = build(build_depther, Config, case)
    x, noise = synthetic.make_inputs(1, case['h'], case['w'], case['randsteps'], 256, 1, seed=case['seed'])
    rec = dict(pred=[], feat=[])
    G.wrap_forward(model.decode_head, rec['pred'])
    hk = model.down.register_forward_hook(lambda mod, i, o: rec['feat'].append(o.clone()))
    with G.RandnPatch(noise[0]):
        out = model.sample(x, None)
    hk.remove()
    # encode_decode's clamp with the HEAD's range (depther/ddp.py:101)
    clamped = torch.clamp(out, min=model.decode_head.min_depth, max=model.decode_head.max_depth)
    save(case['name'], dict(task='depth_bins', **case),
         dict(out=out, out_clamped=clamped, depth_pred_steps=torch.stack(rec['pred']), feat_step0=rec['feat'][0],
              x_fp=G.fingerprint(x), noise_fp=G.fingerprint(noise), weights_fp=synthetic.checksum(sd)))


def gen_head(build_depther, Config, case):
    model, sd = build(build_depther, Config, case)
    feat, _ = synthetic.make_inputs(case['R'], case['h'], case['w'], 1, 256, 1, seed=case['seed'])
    temb = model.time_mlp(torch.tensor([case['t']], dtype=torch.float32))
    out = model.decode_head.forward([feat], temb)
    save(case['name'], dict(task='depth_bins_head', **case),
         dict(out=out, temb=temb, feat_fp=G.fingerprint(feat), weights_fp=synthetic.checksum(sd)))


def main():
    import ref_shim
    build_depther, Config = ref_shim.import_depth()
    torch.set_num_threads(8)
    with torch.no_grad():
        for case in CASES:
            gen_sampler(build_depther, Config, case)
        gen_head(build_depther, Config, HEAD_CASE)


if __name__ == '__main__':
    main()
