"""Shared by the binned-depth / split-range tests: the fixtures of ``tests/golden/depth_bins/`` (made by
``golden/gen_golden_depth_bins.py``), the depther config they were made from, and a CPU restatement of the depth sampler with
the binned head (depth/depth/models/decode_heads/decode_head.py:233-266; depther/ddp.py:229-247) composed from ``oracle.ddp_oracle``
pieces."""
import glob
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from ddp_amd.utils import synthetic
from golden_util import fingerprint
from oracle import ddp_oracle as O

BINS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'depth_bins')

ENCODER = dict(type='DetrTransformerEncoder', num_layers=6,
               transformerlayers=dict(type='BaseTransformerLayer', use_time_mlp=True,
                                      attn_cfgs=dict(type='MultiScaleDeformableAttention', embed_dims=256,
                                                     num_levels=1, num_heads=8, dropout=0.),
                                      ffn_cfgs=dict(type='FFN', embed_dims=256, feedforward_channels=1024,
                                                    ffn_drop=0., act_cfg=dict(type='GELU')),
                                      operation_order=('self_attn', 'norm', 'ffn', 'norm')))
POSENC = dict(type='SinePositionalEncoding', num_feats=128, normalize=True, offset=-0.5)


def sampler_cases():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(BINS_DIR, '*.npz'))
                  if os.path.basename(p) != 'head_forward.npz')


def _n_bins(cfg):
    return cfg['head'].get('n_bins') if cfg['head'].get('classify') else None


def load(name):
    """-> cfg, state_dict, x (1,256,h,w), noise (r,1,h,w) (sampler cases) / feat (R,256,h,w) (head case), arrays."""
    z = np.load(os.path.join(BINS_DIR, name + '.npz'))
    cfg = json.loads(str(z['config']))
    arrays = {k: torch.from_numpy(z[k]) for k in z.files if k != 'config'}
    sd = synthetic.make_state_dict('depth', 1, 6, 256, seed=cfg['seed'] + 100, n_bins=_n_bins(cfg))
    assert abs(synthetic.checksum(sd) - float(arrays['weights_fp'])) <= 1e-9 * abs(float(arrays['weights_fp']))
    if cfg['task'] == 'depth_bins_head':
        feat, _ = synthetic.make_inputs(cfg['R'], cfg['h'], cfg['w'], 1, 256, 1, seed=cfg['seed'])
        assert np.allclose(fingerprint(feat), arrays['feat_fp'].numpy(), rtol=1e-12)
        return cfg, sd, feat, None, arrays
    x, noise = synthetic.make_inputs(1, cfg['h'], cfg['w'], cfg['randsteps'], 256, 1, seed=cfg['seed'])
    assert np.allclose(fingerprint(x), arrays['x_fp'].numpy(), rtol=1e-12)
    assert np.allclose(fingerprint(noise), arrays['noise_fp'].numpy(), rtol=1e-12)
    return cfg, sd, x, noise[0], arrays


def head_of(cfg):
    """The decode head's settings of a case: range (default: the depther's) and the head kwargs."""
    h = dict(classify=False, scale_up=False, use_eps=True, n_bins=None, bins_strategy='UD', norm_strategy='linear',
             min_depth=cfg['min_depth'], max_depth=cfg['max_depth'])
    h.update(cfg['head'])
    return h


def bins_of(head):
    if head['bins_strategy'] == 'UD':
        return torch.linspace(head['min_depth'], head['max_depth'], head['n_bins'])
    return torch.logspace(head['min_depth'], head['max_depth'], head['n_bins'])


def depther_cfg(cfg, **head_over):
    """The drop-in depther's config dict (the KITTI DDP model's hot-path part) for a fixture's case."""
    head = dict(type='DeformableHeadWithTime', in_channels=[256], channels=256, in_index=[0], dropout_ratio=0., scale_up=False,
                min_depth=cfg['min_depth'], max_depth=cfg['max_depth'], use_eps=True, align_corners=False, num_feature_levels=1,
                encoder=ENCODER, positional_encoding=POSENC)
    if 'head' in cfg:
        head.update(cfg['head'])
    head.update(head_over)
    return dict(type='DDP', bit_scale=cfg.get('bit_scale', 0.1), timesteps=cfg.get('timesteps', 1),
                randsteps=cfg.get('randsteps', 1), time_difference=cfg.get('time_difference', 1), min_depth=cfg['min_depth'],
                max_depth=cfg['max_depth'], test_cfg=dict(mode='whole'), decode_head=head)


def depth_pred(mem, sd, head):
    """decode_head.py:233-266 on the encoder output (R,256,h,w)."""
    logit = F.conv2d(mem, sd['decode_head.conv_depth.weight'], sd['decode_head.conv_depth.bias'], padding=1)
    if head['classify']:
        bins = bins_of(head).to(device=mem.device, dtype=mem.dtype)      # (fp64 evaluations: the bin centres follow the map's dtype)
        if head['norm_strategy'] == 'linear':
            p = torch.relu(logit) + 0.1
            p = p / p.sum(dim=1, keepdim=True)
        elif head['norm_strategy'] == 'softmax':
            p = torch.softmax(logit, dim=1)
        else:
            p = torch.sigmoid(logit)
            p = p / p.sum(dim=1, keepdim=True)
        return torch.einsum('ikmn,k->imn', [p, bins]).unsqueeze(dim=1)
    if head['scale_up']:
        return torch.sigmoid(logit) * (head['max_depth'] if head['use_eps'] else 1)
    return torch.relu(logit) + (head['min_depth'] if head['use_eps'] else 0)


def head_forward(feat, temb, sd, head):
    bs, c, h, w = feat.shape
    mem = O.encoder_forward(feat, temb, sd)
    return depth_pred(mem.permute(0, 2, 1).reshape(bs, c, h, w).contiguous(), sd, head)


def sample(x, noise, sd, cfg):
    """depther/ddp.py:229-247 for one image with the case's head; x0 normalised with the DEPTHER's range."""
    head = head_of(cfg)
    r, bit = cfg['randsteps'], cfg['bit_scale']
    lo, hi = cfg['min_depth'], cfg['max_depth']
    xr = x.repeat(r, 1, 1, 1)
    depth_t = noise.clone()
    pred = None
    for t_now, t_next in O.sampling_time_pairs(cfg['timesteps'], cfg.get('time_difference', 1), 0.0):
        times_now = torch.tensor([t_now], dtype=torch.float32)
        times_next = torch.tensor([t_next], dtype=torch.float32)
        feat = F.conv2d(torch.cat([xr, depth_t], dim=1), sd['down.conv.weight'], sd['down.conv.bias'])
        temb = O.time_mlp(times_now.to(x.device), {k: v.to(x.device) for k, v in sd.items() if k.startswith('time_mlp')})
        pred = head_forward(feat, temb, sd, head)
        x0 = ((pred - lo) / (hi - lo) * 2 - 1) * bit
        a_now = O.gamma_cosine(times_now.view(-1, 1, 1, 1)).to(x.device)
        a_next = O.gamma_cosine(times_next.view(-1, 1, 1, 1)).to(x.device)
        x0 = x0.clamp(-bit, bit)
        eps = (1 / (1 - a_now).sqrt()) * (depth_t - a_now.sqrt() * x0)
        depth_t = a_next.sqrt() * x0 + (1 - a_next).sqrt() * eps
    return pred.mean(dim=0, keepdim=True)
