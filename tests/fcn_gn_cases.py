"""Cases and expectation of the GroupNorm convolutions of FCNHeadWithTime (``ddp_fcn_conv`` with bn_w / bn_b set and NULL running
statistics; include/ddp_mi355x.h), stand-alone (HEAD) and inside the sampler loop (LOOP).  Shared by tests/test_fcn_gn_host.py (CPU)
and tests/test_fcn_gn_gpu.py.

The expectation is the oracle's ``fcn_head_forward`` structure (oracle/ddp_oracle.py) with ``F.group_norm(x, 32, gamma, beta, eps)``
in place of the batch norm, per conv whatever norm the state dict holds for it (``gn.*``: GroupNorm, ``bn.*``: eval BatchNorm, none).
It is handed as the ``head=`` callable to the oracle's ``ddim_sample_seg`` / ``ddpm_sample_seg`` unchanged.

Shapes are the smallest at which the new code can still go wrong: the statistics take the fused route (the stream GEMM's epilogue
writes partial sums per wave of 32 tokens) exactly when h * w % 32 == 0, else the stand-alone pass; a map of one pixel has 8 values
per group; 24 x 24 x 3 spans seven tiles of 256 tokens; several tiny maps share one block of the apply kernel (128 tokens, the affine
of two maps in LDS, further maps folded in registers)."""
import ctypes as C

import torch
import torch.nn.functional as F

from ddp_amd import _lib, schedule
from ddp_amd.utils import synthetic
from oracle import ddp_oracle as O
from support import REL, FcnLoop  # noqa: F401  (REL: the project's bar, restated by test_fcn_gn_host.py::test_bars)

F32_VS_F64 = 1e-5          # the fp32 expectation against the fp64 one
MARGIN = 1e-3              # loop cases: smallest top-2 margin, as a share of the largest |score| of the step (5 x REL: a decision
#                            cannot flip under two scores each REL off)
APPLY_BLOCK = 128          # tokens per block of k_gn_film_relu_blk (csrc/ddp_fcn_gn.hip: GF_GROUPS x 32)

HEAD = {}


def _head(name, maps, h, w, num_convs=1, dilation=1, classes=19, norms=None, conv_b=False, time=True, eps=1e-5, gamma=None):
    assert name not in HEAD
    HEAD[name] = dict(name=name, seed=1300 + len(HEAD), maps=maps, h=h, w=w, num_convs=num_convs, dilation=dilation, classes=classes,
                      norms=tuple(norms) if norms is not None else ('gn',) * num_convs, conv_b=conv_b, time=time, eps=eps, gamma=gamma)


# non-fused statistics (h * w % 32 != 0)
_head('pixel', 2, 1, 1, num_convs=2, classes=1)
_head('pixels_5', 5, 1, 1, classes=19)                               # five maps in one block of the apply pass
_head('row_1x37', 2, 1, 37, num_convs=2, classes=150)
_head('col_37x1', 1, 37, 1, dilation=2, classes=256)
_head('odd_3maps', 3, 5, 7, num_convs=2, conv_b=True)                # three maps in one block; conv bias together with GN
# fused statistics
_head('wave_4x8', 1, 4, 8, num_convs=2, classes=256)                 # exactly one wave per map
_head('wave_4x8_d3', 2, 4, 8, dilation=3, classes=19)                # dilation 3: rows 0 / 3 see each other, most taps leave the map
_head('waves_8x8', 2, 8, 8, eps=1e-3, classes=150)                   # two waves per map
_head('tiles_24x24', 3, 24, 24, num_convs=2)                         # 1728 tokens: seven tiles, map borders inside tiles and blocks
_head('eight_convs', 2, 4, 8, num_convs=8)
_head('no_convs', 2, 4, 8, num_convs=0)
_head('notime_d2', 1, 10, 14, num_convs=2, dilation=2, time=False)   # the BN twin: tests/golden fcn_bn_dil2_notime
_head('gamma_zeros', 2, 5, 7, num_convs=2, gamma='zeros_and_negative', eps=1e-3)
_head('convb_fused', 2, 8, 8, conv_b=True, classes=1)
_head('mixed_bn_gn_none', 2, 8, 8, num_convs=3, norms=('bn', 'gn', None))
_head('mixed_gn_bn', 2, 5, 7, num_convs=2, norms=('gn', 'bn'))


def fused_route(c):
    return (c['h'] * c['w']) % 32 == 0


def _norm_keys(sd, p, kind, g):
    for k in [k for k in sd if k.startswith(p + 'gn.') or k.startswith(p + 'bn.')]:
        del sd[k]
    if kind == 'bn':
        sd[p + 'bn.weight'] = 1.0 + 0.2 * torch.randn((256,), generator=g)
        sd[p + 'bn.bias'] = 0.1 * torch.randn((256,), generator=g)
        sd[p + 'bn.running_mean'] = 0.2 * torch.randn((256,), generator=g)
        sd[p + 'bn.running_var'] = 0.5 + torch.rand((256,), generator=g)
    if kind is None:
        sd[p + 'conv.bias'] = 0.1 * torch.randn((256,), generator=g)


def head_state(c, prefix=''):
    """the seeded state dict: ``synthetic.make_fcn_state_dict(..., norm='gn')``, then what the case changes"""
    sd = synthetic.make_fcn_state_dict(c['num_convs'], c['classes'], True, False, c['seed'], norm='gn')
    g = torch.Generator().manual_seed(77_000 + c['seed'])
    for i, kind in enumerate(c['norms']):
        p = f'convs.{i}.'
        if kind != 'gn':
            _norm_keys(sd, p, kind, g)
        elif c['conv_b']:
            sd[p + 'conv.bias'] = 0.3 * torch.randn((256,), generator=g) + 0.2
        if kind == 'gn' and c['gamma'] == 'zeros_and_negative':
            ga = sd[p + 'gn.weight'].clone()
            ga[::5] = 0.0                       # exact zeros: the channel is beta * (1 + s) + t
            ga[3] = -1.25                       # a negative entry
            ga[8:16] = 0.0                      # a whole group
            sd[p + 'gn.weight'] = ga
    return {prefix + k: v for k, v in sd.items()}


def head_inputs(c):
    feat, temb = synthetic.make_fcn_inputs(c['maps'], c['h'], c['w'], c['seed'])
    return feat, (temb if c['time'] else None)


def expect_head(feat, temb, sd, num_convs, dilation=1, eps=1e-5, prefix='', tap=None):
    """oracle.fcn_head_forward with GroupNorm(32) where the conv has ``gn.*`` keys.  ``tap(i, conv_out, normed)``: optional witness"""
    x = feat
    for i in range(num_convs):
        p = f'{prefix}convs.{i}.'
        x = F.conv2d(x, sd[p + 'conv.weight'], sd.get(p + 'conv.bias'), padding=dilation, dilation=dilation)
        y = x
        if p + 'gn.weight' in sd:
            x = F.group_norm(x, 32, sd[p + 'gn.weight'], sd[p + 'gn.bias'], eps)
        elif p + 'bn.weight' in sd:
            x = F.batch_norm(x, sd[p + 'bn.running_mean'], sd[p + 'bn.running_var'], sd[p + 'bn.weight'], sd[p + 'bn.bias'], False, 0.0, 1e-5)
        if tap is not None:
            tap(i, y, x)
        if temb is not None:
            te = F.linear(F.silu(temb), sd[p + 'time_mlp.1.weight'], sd[p + 'time_mlp.1.bias'])
            scale, shift = te[:, :, None, None].chunk(2, dim=1)
            x = x * (scale + 1) + shift
        x = F.relu(x)
    return F.conv2d(x, sd[prefix + 'conv_seg.weight'], sd[prefix + 'conv_seg.bias'])


def cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


_HEAD_EXPECT = {}


def head_expect(c, dtype=torch.float32):
    key = (c['name'], dtype)
    if key not in _HEAD_EXPECT:
        feat, temb = head_inputs(c)
        with torch.no_grad():
            _HEAD_EXPECT[key] = expect_head(feat.to(dtype), temb.to(dtype) if temb is not None else None, cast(head_state(c), dtype),
                                            c['num_convs'], c['dilation'], c['eps'])
    return _HEAD_EXPECT[key]


def head_query(lib, c, maps=None):
    n = C.c_size_t(0)
    _lib.check(lib.ddp_fcn_head_workspace(c['maps'] if maps is None else maps, c['h'], c['w'], c['classes'], C.byref(n)), lib)
    return n.value


def conv_array(sd, c, dev, prefix=''):
    """the ddp_fcn_conv array of a case straight from its state dict (any mixture of norms) -> (array, tensors kept alive)"""
    keep = []

    def ptr(key):
        t = sd.get(prefix + key)
        if t is None:
            return None
        t = t.detach().float().contiguous().to(dev)
        keep.append(t)
        return t.data_ptr()
    arr = (_lib.DdpFcnConv * max(c['num_convs'], 1))()
    for i in range(c['num_convs']):
        p = f'convs.{i}.'
        arr[i].conv_w, arr[i].conv_b = ptr(p + 'conv.weight'), ptr(p + 'conv.bias')
        if prefix + p + 'gn.weight' in sd:
            arr[i].bn_w, arr[i].bn_b, arr[i].bn_mean, arr[i].bn_var, arr[i].bn_eps = ptr(p + 'gn.weight'), ptr(p + 'gn.bias'), None, None, c['eps']
        else:
            arr[i].bn_w, arr[i].bn_b = ptr(p + 'bn.weight'), ptr(p + 'bn.bias')
            arr[i].bn_mean, arr[i].bn_var, arr[i].bn_eps = ptr(p + 'bn.running_mean'), ptr(p + 'bn.running_var'), 1e-5
        arr[i].time_w, arr[i].time_b = ptr(p + 'time_mlp.1.weight'), ptr(p + 'time_mlp.1.bias')
    return arr, keep


# ---- the sampler loop ----------------------------------------------------------------------------------------------------------
LOOP = {}


def _loop(name, seed, **kw):
    c = dict(name=name, seed=seed, B=1, r=1, K=3, sampler='ddim', classes=19, h=4, w=8, Cx=256, num_convs=2, dilation=1,
             norms=None, conv_b=False, time=True, eps=1e-5, gamma=None, accumulation=True, bit_scale=0.01, td=1)
    c.update(kw)
    c['norms'] = tuple(c['norms']) if c['norms'] is not None else ('gn',) * c['num_convs']
    assert name not in LOOP
    LOOP[name] = c


# seeds: the first from the base for which the fp64 expectation keeps MARGIN at every pixel and step (test_fcn_gn_host.py asserts it)
_loop('b1_ddim_fused', 2000, B=1, r=1)                                                   # B * r = 1
_loop('b2_ddpm_odd', 2106, B=2, r=1, h=5, w=7, sampler='ddpm')                           # B * r = 2, non-fused statistics
_loop('b2_r2_ddim', 2215, B=2, r=2, h=8, w=4, K=2, accumulation=False)                   # B * r = 2 x 2
_loop('r2_ddpm_mixed', 2301, B=1, r=2, h=3, w=5, sampler='ddpm', norms=('bn', 'gn'))     # a BN conv (per-step images) beside a GN conv
_loop('b2_ddim_eps', 2416, B=2, r=1, h=4, w=8, eps=1e-3, num_convs=1, dilation=2)


def loop_state(c):
    sd = {k: v for k, v in synthetic.make_state_dict('seg', c['classes'], 0, c['Cx'], seed=c['seed']).items()
          if not k.startswith('decode_head.')}
    sd.update(head_state(c, prefix='decode_head.'))
    return sd


def loop_inputs(c):
    """-> x (B,Cx,h,w), noise (B,r,256,h,w), step_noise (K,B,r,256,h,w) or None"""
    x, noise = synthetic.make_inputs(c['B'], c['h'], c['w'], c['r'], c['Cx'], 256, seed=c['seed'] + 1)
    sn = None
    if c['sampler'] == 'ddpm':
        g = torch.Generator().manual_seed(c['seed'] + 2)
        sn = torch.randn((c['K'], c['B'], c['r'], 256, c['h'], c['w']), generator=g)
    return x, noise, sn


def loop_cfg(c, batch=None, flags=0):
    cfg = _lib.DdpCfg()
    cfg.abi_version = _lib.ABI_VERSION
    cfg.task = _lib.TASK_SEG
    cfg.sampler = _lib.SAMPLER_DDPM if c['sampler'] == 'ddpm' else _lib.SAMPLER_DDIM
    cfg.batch, cfg.randsteps, cfg.timesteps, cfg.num_layers = (c['B'] if batch is None else batch), c['r'], c['K'], 0
    cfg.num_classes, cfg.feat_channels = c['classes'], c['Cx']
    cfg.h = cfg.head_h = c['h']
    cfg.w = cfg.head_w = c['w']
    cfg.accumulation, cfg.bit_scale = int(bool(c['accumulation'])), c['bit_scale']
    cfg.gemm_mode = _lib.GEMM_BF16X3
    cfg.flags = flags
    return cfg


def loop_steps(c):
    recs = schedule.step_records('seg', c['K'], c['td'], 0.0, 'cosine', c['sampler'])
    steps = (_lib.DdpStep * c['K'])()
    for i, r in enumerate(recs):
        for k, v in r.items():
            setattr(steps[i], k, v)
    return steps


def loop_query(lib, c, batch=None, flags=0):
    n = C.c_size_t(0)
    cfg = loop_cfg(c, batch, flags)
    _lib.check(lib.ddp_sample_fcn_workspace(C.byref(cfg), c['num_convs'], c['dilation'], C.byref(n)), lib)
    return n.value


def run_loop(c, sd, x, noise, sn, dtype=torch.float32):
    """the oracle's sampler around expect_head, one image per run -> (out (B,classes,h,w), logits per image and step [(r,classes,h,w)])"""
    sd = cast(sd, dtype)
    kw = dict(timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'], time_difference=c['td'], accumulation=c['accumulation'])
    outs, steps = [], []
    with torch.no_grad():
        for b in range(x.shape[0]):
            seen = []

            def head(feat, temb):
                seen.append(expect_head(feat, temb, sd, c['num_convs'], c['dilation'], c['eps'], 'decode_head.'))
                return seen[-1]
            xb, nb = x[b:b + 1].to(dtype), noise[b].to(dtype)
            if c['sampler'] == 'ddpm':
                outs.append(O.ddpm_sample_seg(xb, nb, sn[:, b].to(dtype), sd, head=head, **kw))
            else:
                outs.append(O.ddim_sample_seg(xb, nb, sd, head=head, **kw))
            steps.append(seen)
    return torch.cat(outs, dim=0), steps


_LOOP_EXPECT = {}


def loop_expect(c, dtype=torch.float32):
    key = (c['name'], dtype)
    if key not in _LOOP_EXPECT:
        _LOOP_EXPECT[key] = run_loop(c, loop_state(c), *loop_inputs(c), dtype=dtype)
    return _LOOP_EXPECT[key]


def loop_decisions(steps):
    """[image][step] logits (r,classes,h,w) -> (K, B, r, h, w) uint8, the layout of the step record"""
    return torch.stack([torch.stack([s.argmax(1) for s in img]) for img in steps], dim=1).to(torch.uint8)


def loop_min_margin(steps):
    """smallest top-2 margin over every image, step and pixel, as a share of the step's largest |score|"""
    worst = float('inf')
    for img in steps:
        for s in img:
            t = s.topk(2, dim=1).values
            worst = min(worst, float((t[:, 0] - t[:, 1]).min() / s.abs().max()))
    return worst


# the reference fixtures (tests/golden/gen_fcn_gn_golden.py): name -> the generator's case; inputs and weights from the seeds
FIXTURE_HEADS = ('fcn_gn_2conv', 'fcn_gn_dil2_notime')
FIXTURE_LOOPS = ('loopfcn_gn_k3', 'loopfcn_gn_ddpm_r2')


def _golden(name):
    import json
    import numpy as np
    from golden_util import GOLDEN_DIR, fingerprint
    import os
    z = np.load(os.path.join(GOLDEN_DIR, 'fcn_gn', name + '.npz'))
    return json.loads(str(z['config'])), z, fingerprint


def load_fixture_head(name):
    """-> (case dict in HEAD's form, feat, temb or None, state dict, the reference's output)"""
    import numpy as np
    g, z, fingerprint = _golden(name)
    assert g['norm'] == 'gn'
    sd = synthetic.make_fcn_state_dict(g['num_convs'], g['num_classes'], True, g['concat_input'], g['seed'], norm='gn')
    feat, temb = synthetic.make_fcn_inputs(g['maps'], g['h'], g['w'], g['seed'])
    assert abs(synthetic.checksum(sd) - float(z['weights_fp'])) <= 1e-9 * abs(float(z['weights_fp']))
    assert np.allclose(fingerprint(feat), z['feat_fp'], rtol=1e-12)
    c = dict(name=name, seed=g['seed'], maps=g['maps'], h=g['h'], w=g['w'], num_convs=g['num_convs'], dilation=g['dilation'],
             classes=g['num_classes'], norms=('gn',) * g['num_convs'], conv_b=False, time=g['with_time'], eps=1e-5, gamma=None,
             concat_input=g['concat_input'])
    return c, feat, (temb if g['with_time'] else None), sd, torch.from_numpy(z['out'])


def load_fixture_loop(name):
    """-> (case dict in LOOP's form, state dict, x (1,256,h,w), noise (1,r,256,h,w), step noise (K,1,r,256,h,w) or None,
    the reference's output (1,classes,h,w), its logits per step (K,r,classes,h,w))"""
    import numpy as np
    g, z, fingerprint = _golden(name)
    assert g['norm'] == 'gn'
    sd = synthetic.make_fcn_segmentor_state_dict(g['num_convs'], g['num_classes'], True, g['concat_input'], g['seed'] + 100, norm='gn')
    x, noise = synthetic.make_inputs(1, g['h'], g['w'], g['randsteps'], 256, 256, seed=g['seed'])
    assert abs(synthetic.checksum(sd) - float(z['weights_fp'])) <= 1e-9 * abs(float(z['weights_fp']))
    assert np.allclose(fingerprint(x), z['x_fp'], rtol=1e-12) and np.allclose(fingerprint(noise), z['noise_fp'], rtol=1e-12)
    sn = None
    if g['diffusion'] == 'ddpm':
        gen = torch.Generator().manual_seed(g['seed'] + 7)
        sn = torch.randn((g['timesteps'], g['randsteps'], 256, g['h'], g['w']), generator=gen)[:, None]
    c = dict(name=name, seed=g['seed'], B=1, r=g['randsteps'], K=g['timesteps'], sampler=g['diffusion'], classes=g['num_classes'],
             h=g['h'], w=g['w'], Cx=256, num_convs=g['num_convs'], dilation=g['dilation'], norms=('gn',) * g['num_convs'], conv_b=False,
             time=True, eps=1e-5, gamma=None, accumulation=g['accumulation'], bit_scale=g['bit_scale'], td=1)
    return c, sd, x, noise, sn, torch.from_numpy(z['out']), torch.from_numpy(z['logits_steps'])


# ---- what the feature must not change --------------------------------------------------------------------------------------------
def workspace_bytes(lib):
    """both workspace queries on every case -> {'head/<name>': bytes, 'loop/<name>[/rec|/seeded]': bytes}"""
    out = {}
    for n, c in HEAD.items():
        out['head/' + n] = head_query(lib, c)
        out['head1/' + n] = head_query(lib, c, maps=1)
    for n, c in LOOP.items():
        out['loop/' + n] = loop_query(lib, c)
        out['loop1/' + n] = loop_query(lib, c, batch=1)
        out['loop/' + n + '/rec'] = loop_query(lib, c, flags=_lib.FLAG_STEP_RECORD)
        out['loop/' + n + '/seeded'] = loop_query(lib, c, flags=_lib.FLAG_SEEDED_NOISE)
    return out


def unchanged_path_hashes(dev):
    """sha256 of what the BatchNorm / norm-free heads give on the existing fcn_* / loopfcn_* fixtures with the library in use
    (DDP_LIB_PATH or the in-tree build): {fixture: hex}.  tests/golden/fcn_gn/parent_bits.json holds them for the parent's build."""
    import hashlib
    import ddp_amd
    from golden_util import case_names, load_fcn_case, load_loopfcn_case
    out = {}

    def sha(t):
        return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    for name in case_names('fcn'):
        cfg, feat, temb, sd, _ = load_fcn_case(name)
        head = ddp_amd.FCNHeadWithTime(num_convs=cfg['num_convs'], kernel_size=3, concat_input=cfg['concat_input'], dilation=cfg['dilation'],
                                       in_channels=256, channels=256, num_classes=cfg['num_classes'], in_index=0,
                                       norm_cfg=dict(type='BN') if cfg['with_norm'] else None)
        head.load_state_dict(sd, strict=True)
        head = head.to(dev).eval()
        out[name] = sha(head([feat.to(dev)], temb.expand(cfg['maps'], 1024).to(dev) if temb is not None else None))
    for name in case_names('loopfcn'):
        cfg, sd, x, noise, step_noise, _ = load_loopfcn_case(name)
        model = ddp_amd.build_segmentor(dict(
            type='DDP', timesteps=cfg['timesteps'], randsteps=cfg['randsteps'], bit_scale=cfg['bit_scale'],
            accumulation=cfg['accumulation'], diffusion=cfg['diffusion'],
            decode_head=dict(type='FCNHeadWithTime', num_convs=cfg['num_convs'], concat_input=cfg['concat_input'],
                             dilation=cfg['dilation'], in_channels=256, channels=256, num_classes=cfg['num_classes'], in_index=0,
                             norm_cfg=dict(type='BN') if cfg['with_norm'] else None)))
        model.load_state_dict(sd, strict=True)
        model = model.to(dev).eval()
        dn = noise.unsqueeze(0).contiguous().to(dev)
        if cfg['diffusion'] == 'ddpm':
            out[name] = sha(model.ddpm_sample(x.to(dev), noise=dn, step_noise=step_noise.unsqueeze(1).contiguous().to(dev)))
        else:
            out[name] = sha(model.ddim_sample(x.to(dev), noise=dn))
    return out


def device_loop(c, sd, dev, batch=None, flags=0):
    """ddp_prepare_fcn / ddp_sample_fcn through the C ABI on a guarded, exactly sized workspace; the conv array from the state dict"""
    B = c['B'] if batch is None else batch
    return FcnLoop(c, sd, dev, B, conv_array(sd, c, dev, prefix='decode_head.'), loop_cfg(c, B, flags), loop_steps(c),
                   loop_query(_lib.load(), c, B, flags), 'fcn_gn loop')
