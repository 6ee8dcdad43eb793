"""DDP_FLAG_DDPM_CHAIN: the cases tests/test_ddpm_chain_host.py (CPU) and tests/test_ddpm_chain_gpu.py (GPU) share.

A case is a dict in the style of tests/config_space_cases.py: seg, ddpm, cosine schedule, bit_scale 0.01, L = 2, Cx = 256,
Kc = 19, accumulation on, time_difference 1 unless stated.  Each one is about a place where the chain can go wrong:

  dc_k2_td0            K 2, td 0: c rounds to exactly 1.0f at step 0, so ua' = ((1 - c) / alpha) alpha' == 0 - the pre-pass runs with a
                       zero factor on U (and a formulation that divides by ua' would not exist)
  dc_15tok             3 x 5 maps, B 2, Kc 3: one partial 32-token group per call, images straddle it
  dc_1x37_r2_cx96      r 2, Cx 96, Kc 150, no accumulation: step-prologue head (no head7), res_rn, three 64-class chunks
  dc_1x257             one token past a 256-token tile
  dc_kc65_r2_nonoise   K 2, td 1: no step adds noise - the chain runs on the scalars (ua', uc') alone, no pre-pass
  dc_kc256             256 classes (four chunks), no accumulation
  dc_k64               DDP_MAX_STEPS: 63 pre-passes, the regrouping's rounding accumulates over 63 updates
  dc_L1                one layer: the layer + tail kernel is the step's only layer
  dc_sr01              sample_range0 = 0.1: EVERY step has ddpm_add_noise = 1, the last one included - which the chain must skip
                       (the reference computes a mask_t there that nobody reads)

``oracle_batch`` is config_space_cases.oracle_image, except for sample_range0 != 0, which that helper does not forward."""
import numpy as np
import torch

import config_space_cases as S
from ddp_amd import _lib, schedule
from golden_util import max_rel
from oracle import ddp_oracle as O

REL, COND = S.REL, S.COND
CHAIN_VS_CLEAR = 5e-5        # the bar of this regrouping under teacher forcing (tests/test_hip_parity.py uses it for the bev / depth pairs)

CASES = {}


def _add(name, **kw):
    c = dict(name=name, family='ddpm_chain', task='seg', sampler='ddpm', B=1, r=1, K=3, L=2, Cx=256, td=1, Kc=19, bit_scale=0.01,
             accumulation=True, sample_range0=0.0, seed=len(CASES) + 1200)
    c.update(kw)
    assert name not in CASES and name not in S.CASES
    CASES[name] = c


_add('dc_k2_td0', K=2, td=0, h=5, w=7)
_add('dc_15tok', K=3, td=0, B=2, h=3, w=5, Kc=3)
_add('dc_1x37_r2_cx96', K=4, r=2, h=1, w=37, Kc=150, Cx=96, accumulation=False)
_add('dc_1x257', K=3, h=1, w=257, Kc=64)
_add('dc_kc65_r2_nonoise', K=2, td=1, B=2, r=2, h=7, w=13, Kc=65)
_add('dc_kc256', K=3, td=0, h=6, w=9, Kc=256, accumulation=False)
_add('dc_k64', K=64, td=0, h=5, w=6)
_add('dc_L1', K=3, td=0, L=1, h=5, w=7)
_add('dc_sr01', K=3, td=0, h=5, w=7, sample_range0=0.1)

# noise-adding steps the chain runs a pre-pass for / K (the issue's table; asserted against the schedule on the CPU)
NOISE_STEPS = {'dc_k2_td0': (1, 2), 'dc_15tok': (2, 3), 'dc_1x37_r2_cx96': (2, 4), 'dc_1x257': (1, 3), 'dc_kc65_r2_nonoise': (0, 2),
               'dc_kc256': (2, 3), 'dc_k64': (63, 64), 'dc_L1': (2, 3), 'dc_sr01': (2, 3), 'seg_ddpm_acc': (1, 3), 'seg_ddpm_noacc': (1, 3)}

# the two ddpm cases of the configuration sweep run the chain as well
ALL = dict(CASES)
for _n in ('seg_ddpm_acc', 'seg_ddpm_noacc'):
    ALL[_n] = dict(S.CASES[_n], sample_range0=0.0)


def records(c):
    return schedule.step_records('seg', c['K'], c['td'], c['sample_range0'], 'cosine', 'ddpm')


def steps_of(c):
    steps = (_lib.DdpStep * c['K'])()
    for i, r in enumerate(records(c)):
        for k, v in r.items():
            setattr(steps[i], k, v)
    return steps


def chain_scalars(rec):
    """(ua', uc') of a step as sample_seg forms them: fp32, ua' = ((1 - c) / alpha) alpha_next, uc' = c alpha_next"""
    f = np.float32
    c, a, an = f(rec['ddpm_c']), f(rec['alpha']), f(rec['alpha_next'])
    return f(f(f(1) - c) / a) * an, c * an


def prepasses(c):
    """launches of k_u_noise in one call: the noise-adding steps that have a next step"""
    return sum(1 for r in records(c)[:-1] if r['ddpm_add_noise'])


def engine_kwargs(c):
    kw = S.engine_kwargs(c)
    kw['sample_range0'] = c['sample_range0']
    return kw


def make_cfg(c, chain=True, gemm='bf16x3', **flags):
    cfg = S.make_cfg(c, gemm, **flags)
    if chain:
        cfg.flags |= _lib.FLAG_DDPM_CHAIN
    return cfg


_ORACLE = {}


def oracle_batch(c, dtype=torch.float32):
    """(B, Kc, h, w) expectation, image by image, once per (case, dtype) and process"""
    key = (c['name'], dtype)
    if key not in _ORACLE:
        sd = S.state_dict(c)
        x, noise, sn = S.inputs(c)
        outs = []
        for b in range(c['B']):
            if c['sample_range0'] == 0.0:
                outs.append(S.oracle_image(c, sd, x, noise, sn, b, dtype))
                continue
            sdt = {k: v.to(dtype) for k, v in sd.items()}
            with torch.no_grad():
                outs.append(O.ddpm_sample_seg(x[b:b + 1].to(dtype), noise[b].to(dtype), sn[:, b].to(dtype), sdt, timesteps=c['K'],
                                              randsteps=c['r'], bit_scale=c['bit_scale'], time_difference=c['td'],
                                              sample_range0=c['sample_range0'], accumulation=c['accumulation']))
        _ORACLE[key] = torch.cat(outs, dim=0)
    return _ORACLE[key]


# ---- what the GPU file shares with tests/workspace_history_cases.py -----------------------------------------------------------------
VIDS = {'chain': {}, 'chain-unfused-tail': dict(fused_tail=False)}


def check_against_oracle(c, out, label):
    ref = oracle_batch(c)
    assert out.shape == ref.shape and torch.isfinite(out).all(), label
    errs = [max_rel(out[b:b + 1], ref[b:b + 1]) for b in range(c['B'])]
    agree = float((out.argmax(1) == ref.argmax(1)).float().mean())
    print(f'DDPM-CHAIN {label}: max-rel per image {" ".join(f"{e:.3e}" for e in errs)} (bar {REL:.0e}), decisions equal {agree:.4f}')
    assert max(errs) < REL and agree > 0.999
