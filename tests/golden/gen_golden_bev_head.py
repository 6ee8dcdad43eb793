#!/usr/bin/env python
"""Golden vectors of the BEV head's two constructor variants - the 3x3 ``conv_seg`` (``seg_conv_kernel=3``) and
``grid_transform.prescale_factor`` - made BY THE REFERENCE ITSELF.

Run by hand in the build container (needs the reference tree, see ``ref_shim``):

    python tests/golden/gen_golden_bev_head.py [case ...]

The reference's ``DeformableHeadWithTime`` and ``DDP`` (bev/mmdet3d) are built as ``gen_golden.gen_bev`` builds them, loaded with
the seeded synthetic hot-path weights of ``ddp_amd.utils.synthetic`` (``seg_conv_kernel`` selects the (K,256,3,3) conv_seg) and run
with the seeded start noise in place of the in-method ``torch.randn``.  The fixtures go to ``tests/golden/bev_head/`` - NOT the top
level, whose ``bev_*`` files the 1x1 tests enumerate - one ``<case>.npz`` each: the config, input fingerprints, the output, the
head's output of every step, and the smallest |prob - threshold| over all steps and pixels.

The x0 feedback thresholds a probability (fusion_models/ddp.py:290): the loop's only discontinuity.  A case's seed is accepted only
if that smallest distance is >= MIN_MARGIN, so that no implementation within the suite's tolerance can take another decision and
no test has to leave a pixel out; ``seed`` is the first of seed0, seed0 + 1, ... that qualifies.
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
sys.path.insert(0, os.path.dirname(HERE))

import gen_golden as G  # noqa: E402
import bev_head_util as U  # noqa: E402
from ddp_amd.utils import synthetic  # noqa: E402

OUT = os.path.join(HERE, 'bev_head')
MIN_MARGIN = 1e-3
IN16 = [[-51.2, 51.2, 6.4], [-51.2, 51.2, 6.4]]


def grid(step):          # head grid of len(arange(-50 + step / 2, 50, step)) squared: 5.0 -> 20, 8.0 -> 12, 10.0 -> 10
    return dict(input_scope=IN16, output_scope=[[-50, 50, step], [-50, 50, step]])


# seg_gain: see bev_head_util.state_dict_of.  The head grids are kept small enough (<= 7200 probabilities per run) for a seed with
# every probability >= MIN_MARGIN off the threshold to exist among the first few tried.
COMMON = dict(h=16, w=16, feat_channels=256, timesteps=3, bit_scale=0.01, num_layers=4, seg_gain=16.0)
CASES = [
    dict(COMMON, name='seg3_r1', randsteps=1, seed0=300, seg_conv_kernel=3, **grid(5.0)),
    dict(COMMON, name='seg3_r4', randsteps=4, seed0=320, seg_conv_kernel=3, **grid(10.0)),
    dict(COMMON, name='prescale_2', randsteps=1, seed0=340, prescale_factor=2, **grid(5.0)),
    dict(COMMON, name='prescale_05', randsteps=2, seed0=360, prescale_factor=0.5, **grid(8.0)),
    # odd-sized rectangular map: floor(13 * 1.5) = 19, floor(9 * 1.5) = 13 - the size ratio differs from the factor
    dict(COMMON, name='prescale_15_odd', h=13, w=9, randsteps=1, seed0=380, prescale_factor=1.5,
         input_scope=[[-51.2, 51.2, 7.876923076923077], [-51.2, 51.2, 11.377777777777778]],
         output_scope=[[-50, 50, 4.0], [-50, 50, 6.25]]),
    # a factor float32 cannot hold: floor(10 * 0.9) = 9 in the reference's double arithmetic, 8 with float32(0.9)
    dict(COMMON, name='prescale_09_w10', h=12, w=10, randsteps=1, seed0=440, prescale_factor=0.9,
         input_scope=[[-51.2, 51.2, 8.533333333333333], [-51.2, 51.2, 10.24]], output_scope=[[-50, 50, 5.0], [-50, 50, 5.0]]),
    dict(COMMON, name='seg3_prescale_2_fusion', feat_channels=512, randsteps=2, seed0=400, seg_conv_kernel=3, prescale_factor=2,
         **grid(8.0)),
]
HEAD_CASE = dict(name='head_forward', h=16, w=16, R=2, num_layers=4, seed=420, t=0.4, seg_conv_kernel=3, seg_gain=16.0, **grid(5.0))


def save(name, cfg, arrays):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + '.npz')
    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrays.items()}
    np.savez_compressed(path, config=np.array(json.dumps(cfg)), **arrays)
    print(f'wrote {path}  ({os.path.getsize(path) / 1e6:.3f} MB)')


def build(ddp_mod, head_mod, case):
    from mmcv.utils import ConfigDict
    kw = U.head_kwargs(case)
    kw['encoder'] = ConfigDict(kw['encoder'])
    kw['positional_encoding'] = ConfigDict(kw['positional_encoding'])
    head = head_mod.DeformableHeadWithTime(**kw).eval()
    model = ddp_mod.DDP(bit_scale=case.get('bit_scale', 0.01), timesteps=case.get('timesteps', 1),
                        randsteps=case.get('randsteps', 1), feat_channels=case.get('feat_channels', 256)).eval()
    sd = U.state_dict_of(case)
    res = model.load_state_dict({k: v for k, v in sd.items() if not k.startswith('decode_head.')}, strict=False)
    assert not res.unexpected_keys and not res.missing_keys, res
    head.load_state_dict({k[len('decode_head.'):]: v for k, v in sd.items() if k.startswith('decode_head.')}, strict=True)
    return model, head, sd


def gen_sampler(ddp_mod, head_mod, case):
    for seed in range(case['seed0'], case['seed0'] + 60):
        c = dict(case, seed=seed)
        model, head, sd = build(ddp_mod, head_mod, c)
        x, noise = synthetic.make_inputs(1, c['h'], c['w'], c['randsteps'], c['feat_channels'], 256, seed=seed)
        probs = []
        hk = head.register_forward_hook(lambda mod, i, o: probs.append(o.clone()))
        with G.RandnPatch(noise[0]):
            out = model.ddim_sample([x], head)
        hk.remove()
        probs = torch.stack(probs)
        margin = float((probs - model.threshold).abs().min())
        print(f'{c["name"]}: seed {seed} smallest |prob - threshold| {margin:.3e}')
        if margin >= MIN_MARGIN:
            break
    assert margin >= MIN_MARGIN, (case['name'], margin)
    save(c['name'], dict(task='bev_head', **c),
         dict(out=out, prob_steps=probs, thr_margin=margin, x_fp=G.fingerprint(x), noise_fp=G.fingerprint(noise),
              weights_fp=synthetic.checksum(sd)))


def gen_head(ddp_mod, head_mod, case):
    model, head, sd = build(ddp_mod, head_mod, case)
    feat, _ = synthetic.make_inputs(case['R'], case['h'], case['w'], 1, 256, 256, seed=case['seed'])
    temb = model.time_mlp(torch.tensor([case['t']], dtype=torch.float32))
    out = head.forward([feat], temb)
    save(case['name'], dict(task='bev_head_forward', **case),
         dict(out=out, temb=temb, feat_fp=G.fingerprint(feat), weights_fp=synthetic.checksum(sd)))


def main():
    import ref_shim
    ddp_mod, head_mod = ref_shim.import_bev()
    torch.set_num_threads(8)
    with torch.no_grad():
        only = set(sys.argv[1:])          # case names: regenerate these only
        for case in CASES:
            if not only or case['name'] in only:
                gen_sampler(ddp_mod, head_mod, case)
        if not only or HEAD_CASE['name'] in only:
            gen_head(ddp_mod, head_mod, HEAD_CASE)


if __name__ == '__main__':
    main()
