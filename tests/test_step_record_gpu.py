"""DDP_FLAG_STEP_RECORD on the GPU (``pytest -m gpu``): the per-step record and the step-disagreement map.

Every engine of this file samples through a workspace that starts and ends with a 4 KiB guard and is filled with a NaN pattern
(tests/test_config_space_gpu.py): the two new buffers are the LAST of the workspace, so an overrun lands in the rear guard.
Shapes are that file's small ones: maps of 7 x 13, 5 x 9 and 1 x 37, L = 2, K = 3 (seg, bev) or 4 (depth); the bev head
variants (3x3 conv_seg, prescale) run on the reference-made fixtures of tests/golden/bev_head/ (16 x 16 maps, L = 4, K = 3).

What is checked
  non-interference   `out` with the flag set is bit-identical to `out` with it clear, on every route; with it clear the launch
                     records are the ones tests/test_config_space_gpu.py::_expected lists for the route
  record vs oracle   seg: argmax of the oracle's per-step logits (ddim_sample_seg(trace=)), equal wherever the oracle's top-2 gap
                     exceeds the rule of the seg fixtures, GAP_RULE = 1e-4 x max|logits| of the step (tests/golden/gen_golden.py
                     :794-798, tests/test_full_size_parity.py, tests/test_oracle_golden.py); entries under the rule are at most
                     1 % of a case - a condition on the seeds, see SEG_SEEDS.  depth: the oracle's per-step depth_pred at REL.
                     bev: the fixtures' per-step head outputs `prob_steps` > threshold (thr_margin >= 1e-3 is the fixtures' seed
                     rule: no probability closer than that to the threshold); 9 .. 32 classes: the per-step probabilities of the
                     restatement (tests/bev_head_util.py) on the oracle-driven cases of tests/test_bev_head_gpu.py, same rule
  launch counts      the launches the flag adds carry the profiler tag ddp_sample otherwise leaves unused (0): their number per
                     route is the one include/ddp_mi355x.h and DESIGN 3.3 state
  disagreement map   NumPy evaluation of the three definitions of include/ddp_mi355x.h on the engine's OWN record and output:
                     exact for seg / bev (integer counts, one division), within 4 ulp of the fp64 value for depth
  batching / replay  B = 2 against two single-image calls, hipGraph capture + replay with new inputs: bit-identical
  plugin classes     return_steps=True returns the engine's tensors; the default call returns what it returned before
"""
import numpy as np
import pytest
import torch

import bev_head_util as BU
import config_space_cases as S
import support
from ddp_amd import _lib
from golden_util import max_rel
from oracle import ddp_oracle as O
from support import REL, assert_guards, dev, guard, launch_counts, ref_disagreement  # noqa: F401

pytestmark = pytest.mark.gpu

GAP_RULE = 1e-4         # x max|logits| of the step: the top-2 gap rule of the seg fixtures (tests/golden/gen_golden.py:794-798)
# seg seeds: scanned 900 .. 915 on the CPU for both seg cases below (fp32 oracle against its fp64 run, every step): all 32 runs
# take the same decisions in both precisions and have at most 0.55 % of their (step, replica, pixel) entries under GAP_RULE
# (seed 900: none at r = 1, 0.09 % at r = 2); the first seed of each scan is used
SEG_SEEDS = dict(seg=900, seg_r2=900)

_SEG = dict(S.CASES['seg_L12'], L=2, h=7, w=13, K=3)
_DEPTH = dict(S.CASES['depth_K1'], L=2, K=4)
_BEV = dict(S.CASES['bev_kc5_th0.3'], L=2, K=3, h=5, w=9, threshold=0.5)
CASES = {
    # name: (case, engine flags)                                                     route
    'seg_fused': (dict(_SEG, seed=SEG_SEEDS['seg']), {}),                            # head7, u chain, last layer + tail
    'seg_unfused_tail': (dict(_SEG, seed=SEG_SEEDS['seg']), dict(fused_tail=False)),
    'seg_r2_cx96': (dict(_SEG, r=2, Cx=96, seed=SEG_SEEDS['seg_r2']), {}),           # prologue path, two replicas
    'seg_f32': (dict(_SEG, seed=SEG_SEEDS['seg']), dict(gemm='f32')),                # k_seg_update
    'seg_ddpm': (dict(_SEG, sampler='ddpm', r=2, seed=SEG_SEEDS['seg']), {}),
    'depth_chain': (dict(_DEPTH, h=5, w=9), {}),
    'depth_chain_1x37': (dict(_DEPTH, h=1, w=37, B=3), {}),
    'depth_unfused': (dict(_DEPTH, h=5, w=9), dict(fused_tail=False)),
    'depth_bins': (dict(_DEPTH, h=1, w=37, n_bins=24, norm='softmax'), {}),
    'depth_r2': (dict(_DEPTH, h=5, w=9, r=2), {}),                                   # k_layer MODE 3 step head with the fused update
    'depth_f32': (dict(_DEPTH, h=7, w=13, r=2), dict(gemm='f32')),
    'bev_chain': (dict(_BEV, Kc=6), {}),
    'bev_chain_r2_kc8': (dict(_BEV, Kc=8, r=2), {}),
    'bev_kc9': (dict(_BEV, Kc=9), {}),
    'bev_kc32_r2': (dict(_BEV, Kc=32, r=2), {}),
    'bev_unfused_tail': (dict(_BEV, Kc=6), dict(fused_tail=False)),
}
for _n, (_c, _f) in CASES.items():
    _c['name'] = 'step_record_' + _n
PATHS = {'seg_fused': 'seg_head7', 'seg_r2_cx96': 'seg_prologue', 'seg_unfused_tail': 'seg_unfused_tail_head7', 'depth_chain': 'depth_chain',
         'depth_r2': 'depth_lt', 'depth_bins': 'depth_bins', 'depth_unfused': 'depth_unfused_tail', 'bev_chain': 'bev_chain',
         'bev_kc9': 'bev_separate', 'bev_unfused_tail': 'bev_separate'}
BEV_FIXTURES = ['prescale_05', 'seg3_r4', 'seg3_prescale_2_fusion', 'prescale_15_odd']


def _engine(c, dev, record, batch=None, gemm='bf16x3', **flags):
    return support.engine(S.state_dict(c), c['task'], S.engine_kwargs(c), dev, gemm, batch, record_steps=record, **flags)


_RUNS = {}


def _run(name, dev):
    """-> dict(out, rec, map, plain): one flagged and one plain call of the case, computed once per process"""
    if name not in _RUNS:
        c, flags = CASES[name]
        x, noise, sn = S.inputs(c)
        args = (x.to(dev), noise.to(dev), sn.to(dev) if sn is not None else None)
        plain_eng = _engine(c, dev, False, **flags)
        plain = plain_eng.sample(*args).cpu()
        assert_guards(plain_eng, name)
        eng = _engine(c, dev, True, **flags)
        with pytest.raises(_lib.DdpError, match='sample'):
            eng.step_record()
        with pytest.raises(_lib.DdpError, match='sample'):
            eng.step_disagreement()
        out = eng.sample(*args)
        torch.cuda.synchronize()
        assert_guards(eng, name)
        _RUNS[name] = dict(out=out.cpu(), rec=eng.step_record().cpu(), map=eng.step_disagreement().cpu(), plain=plain, eng=eng, args=args)
    return _RUNS[name]


def _shapes(c):
    hh, wh = S.head_grid(c)
    dtype = dict(seg=torch.uint8, depth=torch.float32, bev=torch.int32)[c['task']]
    return (c['K'], c['B'], c['r'], hh, wh), dtype, (c['B'], hh, wh)


def _assert_map(task, rec, out, got, threshold=0.5):
    want = ref_disagreement(task, rec, out, threshold)
    got = got.numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    if task != 'depth':
        assert np.array_equal(got, want), f'max |diff| {np.abs(got - want).max()}'
        return
    w32 = want.astype(np.float32)
    ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(w32)).astype(np.float64)
    print(f'STEP-RECORD depth map: worst distance from the fp64 value {ulps.max():.2f} ulp (bar 4)')
    assert np.isfinite(got).all() and ulps.max() <= 4.0


# ---- 1. non-interference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_out_is_bit_identical_with_and_without_the_flag(dev, name):
    c, _ = CASES[name]
    r = _run(name, dev)
    shape, dtype, mshape = _shapes(c)
    assert torch.equal(r['out'], r['plain'])
    assert tuple(r['rec'].shape) == shape and r['rec'].dtype == dtype
    assert tuple(r['map'].shape) == mshape and r['map'].dtype == torch.float32
    assert torch.isfinite(r['map']).all()
    if c['K'] * c['r'] > 1 and c['task'] != 'depth':
        assert float(r['map'].max()) <= 1.0 and float(r['map'].min()) >= 0.0


@pytest.mark.parametrize('name', sorted(PATHS))
def test_launch_records_with_the_flag_clear_and_set(dev, name):
    """flag clear: the route's launch counts per tag (tests/test_config_space_gpu.py::_expected); flag set: the same tagged launches -
    the record's own kernels carry no tag"""
    c, flags = CASES[name]
    x, noise, sn = S.inputs(c)
    want = S.expected_launches(PATHS[name], c['K'], c['L'])
    extra = {}
    for record in (False, True):
        eng = _engine(c, dev, record, **flags)
        got = launch_counts(eng, x.to(dev), noise.to(dev), sn.to(dev) if sn is not None else None)
        assert_guards(eng, name)
        assert {t: got[t] for t in want} == want, (name, record, got)
        extra[record] = got[0]
    # the launches the flag adds (tag 0, which no launch of ddp_sample otherwise carries): k_step_disagreement once per call; bev
    # + k_bev_record per step; depth + a head-only k_depth_update per step whose update runs inside the next step's head
    K = c['K']
    added = {'seg': 1, 'bev': K + 1, 'depth': K if PATHS[name] in ('depth_chain', 'depth_lt') else 1}[c['task']]
    assert extra[False] == 0 and extra[True] == added, (name, extra, added)


# ---- 2. the record against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['seg_fused', 'seg_unfused_tail', 'seg_r2_cx96', 'seg_f32'])
def test_seg_record_matches_the_oracles_per_step_argmax(dev, name):
    c, _ = CASES[name]
    rec = _run(name, dev)['rec']
    sd = S.state_dict(c)
    x, noise, _ = S.inputs(c)
    under = total = 0
    for b in range(c['B']):
        trace = []
        with torch.no_grad():
            O.ddim_sample_seg(x[b:b + 1], noise[b], sd, timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'],
                              time_difference=c['td'], accumulation=c['accumulation'], trace=trace)
        for s, t in enumerate(trace):
            lg = t['logits']                                              # (r,Kc,h,w)
            top2 = lg.topk(2, dim=1).values
            clear = (top2[:, 0] - top2[:, 1]) > GAP_RULE * lg.abs().max()
            under += int((~clear).sum())
            total += clear.numel()
            diff = rec[s, b].long() != lg.argmax(1)
            assert not (diff & clear).any(), f'{name}: image {b} step {s}: {int((diff & clear).sum())} decisions differ above the gap rule'
    print(f'STEP-RECORD {name}: {under} of {total} entries under the gap rule ({under / total:.4f}, condition <= 0.01)')
    assert under <= 0.01 * total


@pytest.mark.parametrize('name', ['seg_fused', 'seg_unfused_tail', 'seg_r2_cx96', 'seg_f32', 'seg_ddpm'])
def test_seg_record_is_the_record_x0_trace(dev, name):
    """the same call with DDP_FLAG_RECORD_X0: the same bits, from either flag alone and from both together"""
    from ddp_amd.engine import DDPEngine
    c, flags = CASES[name]
    r = _run(name, dev)
    for record in (False, True):
        eng = guard(DDPEngine(S.state_dict(c), 'seg', device=dev, record_x0=True, record_steps=record,
                              **dict(dict(gemm='bf16x3'), **flags), **S.engine_kwargs(c)))
        out = eng.sample(*r['args'])
        torch.cuda.synchronize()
        assert_guards(eng, name)
        assert torch.equal(out.cpu(), r['out'])
        trace = eng.x0_trace().cpu()                                      # (K, B*r, h, w)
        assert torch.equal(trace.reshape(r['rec'].shape), r['rec'])
        if record:
            assert torch.equal(eng.step_record().cpu(), r['rec']) and torch.equal(eng.step_disagreement().cpu(), r['map'])


@pytest.mark.parametrize('name', ['depth_chain', 'depth_chain_1x37', 'depth_unfused', 'depth_r2', 'depth_f32'])
def test_depth_record_matches_the_oracles_per_step_prediction(dev, name):
    c, _ = CASES[name]
    rec = _run(name, dev)['rec']
    sd = S.state_dict(c)
    x, noise, _ = S.inputs(c)
    for b in range(c['B']):
        trace = []
        with torch.no_grad():
            O.sample_depth(x[b:b + 1], noise[b], sd, timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'], time_difference=c['td'],
                           min_depth=c['min_depth'], max_depth=c['max_depth'], scale_up=c['scale_up'], use_eps=c['use_eps'], trace=trace)
        assert len(trace) == c['K']
        for s, t in enumerate(trace):
            want = t['depth_pred'].reshape(c['r'], c['h'], c['w'])
            err = max_rel(rec[s, b], want)
            assert err < REL, f'{name}: image {b} step {s}: max-rel {err:.3e}'


def test_depth_binned_record_ends_in_the_output(dev):
    """binned head (no per-step oracle trace): the last step's record, averaged over r, IS the output; every step is a valid depth"""
    c, _ = CASES['depth_bins']
    r = _run('depth_bins', dev)
    assert torch.equal(r['rec'][-1].mean(1, keepdim=True), r['out'])
    assert float(r['rec'].min()) >= c['min_depth'] and float(r['rec'].max()) <= c['max_depth']


@pytest.mark.parametrize('name', ['depth_chain', 'depth_r2', 'depth_unfused'])
def test_depth_last_record_gives_the_output(dev, name):
    r = _run(name, dev)
    c, _ = CASES[name]
    assert torch.equal((r['rec'][-1].sum(1, keepdim=True) / c['r']) if c['r'] > 1 else r['rec'][-1], r['out'])


@pytest.mark.parametrize('name', BEV_FIXTURES)
@pytest.mark.parametrize('route', ['default', 'unfused-tail', 'f32'])
def test_bev_record_matches_the_reference_fixtures(dev, name, route):
    """per-step head outputs of the reference (tests/golden/bev_head/*.npz: prob_steps (K,r,6,H,W)) thresholded, against the bits of
    the record - u chain with prescale, 3x3 conv_seg with and without the chain, the separate kernels, the fp32 engine"""
    from ddp_amd.engine import DDPEngine
    cfg, sd, x, noise, g = BU.load(name)
    thr = cfg.get('threshold', 0.5)
    assert float(g['thr_margin']) >= 1e-3
    kw = dict(gemm='f32') if route == 'f32' else dict(gemm='bf16x3', fused_tail=route != 'unfused-tail')
    args = (x.to(dev), noise.unsqueeze(0).contiguous().to(dev))
    plain = guard(DDPEngine(sd, 'bev', device=dev, **kw, **BU.engine_kwargs(cfg))).sample(*args).cpu()
    eng = guard(DDPEngine(sd, 'bev', device=dev, record_steps=True, **kw, **BU.engine_kwargs(cfg)))
    out = eng.sample(*args).cpu()
    assert_guards(eng, name)
    assert torch.equal(out, plain)
    rec, dmap = eng.step_record().cpu(), eng.step_disagreement().cpu()
    want = g['prob_steps'] > thr                                          # (K,r,6,H,W)
    K, r, Kc = want.shape[:3]
    assert tuple(rec.shape) == (K, 1, r) + tuple(want.shape[3:])
    bits = ((rec[:, 0, :, None].long() >> torch.arange(Kc).view(1, 1, Kc, 1, 1)) & 1).bool()
    assert torch.equal(bits, want)
    assert int((rec.long() >> Kc).abs().sum()) == 0                       # no bit above the classes
    _assert_map('bev', rec, out, dmap, thr)


@pytest.mark.parametrize('name,route', [('seg3_kc9', 'default'), ('seg3_kc9', 'f32'), ('seg3_kc32', 'default'), ('seg3_kc32', 'f32'),
                                        ('prescale_2_kc9', 'default'), ('prescale_2_kc9', 'f32'), ('seg3_kc8', 'unfused-tail')])
def test_bev_record_above_eight_classes_matches_the_restatement(dev, name, route):
    """9 .. 32 classes (and 8 on the separate kernels): k_bev_record thresholds the logits rows itself - bit c of every step and
    replica against prob_c > threshold of the restatement's per-step head outputs, c up to 31.  Cases and seeds are those of
    tests/test_bev_head_gpu.py (every probability of every step >= 1e-3 off the threshold; _oracle asserts it)"""
    from ddp_amd.engine import DDPEngine
    cfg = BU.ORACLE_CASES[name]
    sd, x, noise, _ = BU.oracle(cfg)
    trace = BU.ORACLE_REF[(name, 1)][4]
    assert min(t['margin'] for t in trace) >= 1e-3
    thr, Kc = cfg.get('threshold', 0.5), cfg.get('num_classes', 6)
    kw = dict(gemm='f32') if route == 'f32' else dict(gemm='bf16x3', fused_tail=route != 'unfused-tail')
    eng = guard(DDPEngine(sd, 'bev', device=dev, record_steps=True, **kw, **BU.engine_kwargs(cfg)))
    out = eng.sample(x.to(dev), noise.contiguous().to(dev)).cpu()
    assert_guards(eng, name)
    rec, dmap = eng.step_record().cpu(), eng.step_disagreement().cpu()
    want = torch.stack([t['prob'] > thr for t in trace])                 # (K,r,Kc,H,W)
    assert tuple(rec.shape) == (cfg['timesteps'], 1, cfg['randsteps']) + tuple(want.shape[3:])
    bits = ((rec[:, 0, :, None].long() >> torch.arange(Kc).view(1, 1, Kc, 1, 1)) & 1).bool()
    assert torch.equal(bits, want)
    assert bool(want[:, :, 8:].any()) or Kc <= 8                         # (the high bits are exercised: some are set)
    if Kc < 32:
        assert int((rec.long() >> Kc).abs().sum()) == 0
    _assert_map('bev', rec, out, dmap, thr)


# ---- 3. the disagreement map ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_disagreement_map_is_the_definition_applied_to_the_record(dev, name):
    c, _ = CASES[name]
    r = _run(name, dev)
    _assert_map(c['task'], r['rec'], r['out'], r['map'], c.get('threshold', 0.5))


@pytest.mark.parametrize('task', ['seg', 'depth', 'bev'])
def test_single_record_gives_zeros(dev, task):
    base = dict(seg=_SEG, depth=dict(_DEPTH, h=5, w=9), bev=dict(_BEV, Kc=6))[task]
    c = dict(base, K=1, r=1, name='step_record_k1_' + task)
    x, noise, _ = S.inputs(c)
    eng = _engine(c, dev, True)
    out = eng.sample(x.to(dev), noise.to(dev)).cpu()
    assert_guards(eng, c['name'])
    dmap = eng.step_disagreement().cpu()
    if task != 'bev':                      # (bev: out is the step's probability, so its own threshold bits agree as well)
        assert torch.equal(dmap, torch.zeros_like(dmap))
    _assert_map(task, eng.step_record().cpu(), out, dmap, c.get('threshold', 0.5))
    assert torch.equal(dmap, torch.zeros_like(dmap))


# ---- 4. batching and replay -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['seg_fused', 'seg_r2_cx96', 'depth_chain', 'depth_r2', 'depth_bins', 'bev_chain_r2_kc8', 'bev_kc9'])
def test_batched_call_equals_single_image_calls(dev, name):
    c, flags = CASES[name]
    r = _run(name, dev)
    x, noise, _ = S.inputs(c)
    one = _engine(c, dev, True, batch=1, **flags)
    for b in range(c['B']):
        o = one.sample(x[b:b + 1].clone().to(dev), noise[b:b + 1].clone().to(dev)).cpu()
        assert_guards(one, name)
        assert torch.equal(o[0], r['out'][b])
        assert torch.equal(one.step_record().cpu()[:, 0], r['rec'][:, b]), f'{name}: record of image {b}'
        assert torch.equal(one.step_disagreement().cpu()[0], r['map'][b]), f'{name}: map of image {b}'


@pytest.mark.parametrize('name', ['seg_fused', 'depth_chain', 'bev_chain', 'bev_kc9'])
def test_graph_replay_refreshes_record_and_map(dev, name):
    c, flags = CASES[name]
    r = _run(name, dev)
    x, noise, _ = S.inputs(c)
    x2, noise2, _ = S.inputs(dict(c, seed=c['seed'] + 50))
    eng = _engine(c, dev, True, **flags)
    want2 = eng.sample(x2.to(dev), noise2.to(dev)).cpu()
    rec2, map2 = eng.step_record().cpu(), eng.step_disagreement().cpu()
    assert not torch.equal(rec2, r['rec'])                                # the second input does change the record
    graph = eng.capture(x.to(dev), noise.to(dev))
    out = graph.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), r['out'])
    assert torch.equal(eng.step_record().cpu(), r['rec']) and torch.equal(eng.step_disagreement().cpu(), r['map'])
    out = graph.replay(x2.to(dev), noise2.to(dev)).clone()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want2)
    assert torch.equal(eng.step_record().cpu(), rec2) and torch.equal(eng.step_disagreement().cpu(), map2)
    assert_guards(eng, name)


# ---- 5. plugin classes ----------------------------------------------------------------------------------------------------------
def _flag_engine(model):
    engs = [e for e in model._engine_cache.values() if e.cfg.flags & _lib.FLAG_STEP_RECORD]
    assert len(engs) == 1
    return engs[0]


def _check_plugin(model, call, task, threshold=0.5):
    before = call(False).clone()
    got = call(True)
    assert isinstance(got, tuple) and len(got) == 3
    out, rec, dmap = got
    eng = _flag_engine(model)
    assert torch.equal(out, before)
    assert torch.equal(rec, eng.step_record()) and torch.equal(dmap, eng.step_disagreement())
    _assert_map(task, rec.cpu(), out.cpu(), dmap.cpu(), threshold)
    after = call(False)
    assert torch.is_tensor(after) and torch.equal(after, before)          # the default call: a tensor, the same bits
    assert len([e for e in model._engine_cache.values() if not e.cfg.flags & _lib.FLAG_STEP_RECORD]) == 1
    return eng


def test_plugin_segmentor_return_steps(dev):
    from golden_util import load_case
    cfg, sd, x, noise, _, g = load_case('seg_ade_k3')
    model = support.seg_model(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    dx, dn = x.to(dev), noise.unsqueeze(0).to(dev)
    _check_plugin(model, lambda rs: model.ddim_sample(dx, None, noise=dn, return_steps=rs) if rs else model.ddim_sample(dx, None, noise=dn),
                  'seg')
    assert max_rel(model.ddim_sample(dx, None, noise=dn).cpu(), g['out']) < REL


def test_plugin_segmentor_ddpm_return_steps(dev):
    from golden_util import load_case
    cfg, sd, x, noise, step_noise, g = load_case('seg_ddpm')
    model = support.seg_model(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    kw = dict(noise=noise.unsqueeze(0).to(dev), step_noise=step_noise.unsqueeze(1).to(dev))
    _check_plugin(model, lambda rs: model.ddpm_sample(x.to(dev), None, return_steps=rs, **kw) if rs else model.ddpm_sample(x.to(dev), None, **kw),
                  'seg')


def test_plugin_fcn_loop_return_steps(dev):
    """the FCN-head sampler (ddp_sample_fcn): non-interference, record = per-step argmax fed back (equal to the deformable route's
    definition), map, and the same again through a NaN-filled workspace prepared from scratch"""
    import ddp_amd
    from golden_util import load_loopfcn_case
    for name in ('loopfcn_bn_k3', 'loopfcn_nonorm_r2', 'loopfcn_ddpm'):
        cfg, sd, x, noise, step_noise, g = load_loopfcn_case(name)
        model = ddp_amd.build_segmentor(dict(
            type='DDP', timesteps=cfg['timesteps'], randsteps=cfg['randsteps'], bit_scale=cfg['bit_scale'],
            accumulation=cfg['accumulation'], diffusion=cfg['diffusion'],
            decode_head=dict(type='FCNHeadWithTime', num_convs=cfg['num_convs'], concat_input=cfg['concat_input'],
                             dilation=cfg['dilation'], in_channels=256, channels=256, num_classes=cfg['num_classes'], in_index=0,
                             norm_cfg=dict(type='BN') if cfg['with_norm'] else None)))
        model.load_state_dict(sd, strict=True)
        model = model.to(dev).eval()
        dx, dn = x.to(dev), noise.unsqueeze(0).contiguous().to(dev)
        if cfg['diffusion'] == 'ddpm':
            dsn = step_noise.unsqueeze(1).contiguous().to(dev)
            call = lambda rs: model.ddpm_sample(dx, noise=dn, step_noise=dsn, return_steps=rs)       # noqa: E731
        else:
            dsn = None
            call = lambda rs: model.ddim_sample(dx, noise=dn, return_steps=rs)                        # noqa: E731
        eng = _check_plugin(model, call, 'seg')
        out, rec, dmap = call(True)
        assert tuple(rec.shape) == (cfg['timesteps'], 1, cfg['randsteps'], cfg['h'], cfg['w']) and rec.dtype == torch.uint8
        assert max_rel(out.cpu(), g['out']) < REL
        if cfg['accumulation'] is False:                                   # the output is the last step's scores: its argmax is recorded
            if cfg['randsteps'] == 1:
                assert torch.equal(rec[-1, 0, 0].long(), out[0].argmax(0))
        guard(eng)._prepared = False
        again = eng.sample(dx, dn, dsn)
        torch.cuda.synchronize()
        assert_guards(eng, name)
        assert torch.equal(again, out) and torch.equal(eng.step_record(), rec) and torch.equal(eng.step_disagreement(), dmap)


def test_plugin_depther_return_steps(dev):
    from golden_util import load_case
    cfg, sd, x, noise, _, g = load_case('depth_k3_r2')
    model = support.depth_model(cfg, sd)
    dx, dn = x.to(dev), noise.unsqueeze(0).to(dev)
    _check_plugin(model, lambda rs: model.sample(dx, None, noise=dn, return_steps=rs) if rs else model.sample(dx, None, noise=dn), 'depth')
    assert max_rel(model.sample(dx, None, noise=dn).cpu(), g['out']) < REL


def test_plugin_bev_return_steps(dev):
    from golden_util import load_case
    cfg, sd, x, noise, _, g = load_case('bev_fusion')
    model, head = support.bev_plugin(sd, dev, cfg['num_layers'], dict(input_scope=cfg['input_scope'], output_scope=cfg['output_scope']),
                                     bit_scale=cfg['bit_scale'], timesteps=cfg['timesteps'], randsteps=cfg['randsteps'],
                                     feat_channels=cfg['feat_channels'])
    dx, dn = [x.to(dev)], noise.unsqueeze(0).to(dev)
    _check_plugin(model, lambda rs: model.ddim_sample(dx, head, noise=dn, return_steps=rs) if rs else model.ddim_sample(dx, head, noise=dn),
                  'bev', model.threshold)
    assert max_rel(model.ddim_sample(dx, head, noise=dn).cpu(), g['out']) < REL


def test_accessors_refuse_an_engine_without_the_flag(dev):
    c, _ = CASES['seg_fused']
    eng = _engine(c, dev, False)
    x, noise, _ = S.inputs(c)
    eng.sample(x.to(dev), noise.to(dev))
    with pytest.raises(_lib.DdpError, match='record_steps'):
        eng.step_record()
    with pytest.raises(_lib.DdpError, match='record_steps'):
        eng.step_disagreement()
