"""The BEV head's 3x3 ``conv_seg`` and ``grid_transform.prescale_factor`` on the MI355X: every fixture the reference made
(tests/golden/bev_head/) through the plugin classes and through the C ABI under both engines and every diagnostic flag that selects
another route, oracle-driven cases beyond the fixtures (class counts on both sides of the u chain's 8, other factors, a one-row
map, batches, hipGraph replay), and the route of each case read from the library's launch records.  ``pytest -m gpu``.

Every engine of this file samples through a workspace with 4 KiB guards, filled with a NaN pattern (as
tests/test_config_space_gpu.py): a carve() that undersizes a new buffer, or a kernel that reads bytes nobody wrote, shows."""
import pytest
import torch

import ddp_amd  # noqa: F401
from ddp_amd import schedule
from ddp_amd.bev.ddp import DDP as BEVDDP, BEVDeformableHeadWithTime
from ddp_amd.engine import DDPEngine
from ddp_amd.utils import synthetic
import bev_head_util as U
from golden_util import max_rel
from support import REL, assert_guards, guard, launch_counts

pytestmark = pytest.mark.gpu
VARIANTS = {'bf16x3': ('bf16x3', {}), 'f32': ('f32', {}), 'unfused_tail': ('bf16x3', dict(fused_tail=False)),
            'unfused_layer': ('bf16x3', dict(fused_layer=False)), 'gather_guess_zero': ('bf16x3', dict(gather_guess_zero=True))}


def _engine(cfg, sd, gemm='bf16x3', batch=1, **flags):
    return guard(DDPEngine(sd, 'bev', gemm=gemm, **flags, **U.engine_kwargs(cfg, batch)))


def _sample(cfg, sd, x, noise, gemm='bf16x3', **flags):
    eng = _engine(cfg, sd, gemm, batch=x.shape[0], **flags)
    out = eng.sample(x.cuda().contiguous(), noise.cuda().contiguous())
    torch.cuda.synchronize()
    assert_guards(eng, cfg.get('name'))
    return out.cpu()


# ---- the reference-made fixtures --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', sorted(VARIANTS))
@pytest.mark.parametrize('name', U.sampler_cases())
def test_ddp_sample_matches_reference(name, variant):
    cfg, sd, x, noise, g = U.load(name)
    gemm, flags = VARIANTS[variant]
    out = _sample(cfg, sd, x, noise.unsqueeze(0), gemm, **flags)
    assert out.shape == g['out'].shape and torch.isfinite(out).all()
    err = max_rel(out, g['out'])
    print(f'BEV-HEAD {name}[{variant}]: max-rel {err:.3e} (bar {REL:.0e})')
    assert err < REL


def _step_probs(cfg, sd, x, masks, s, gemm):
    """the head's output of step `s` of the case's schedule for the noisy maps `masks` (r,256,h,w) entering it, map by map: a
    one-step engine over a batch of r single maps whose one ddp_step record is step s of the K-step schedule -> (r,K_cls,H,W)"""
    r = masks.shape[0]
    eng = _engine(dict(cfg, timesteps=1, randsteps=1), sd, gemm, batch=r)
    recs = schedule.step_records('bev', cfg['timesteps'], cfg.get('time_difference', 1), 0.0, 'cosine', 'ddim')
    for k, v in recs[s].items():
        setattr(eng.steps[0], k, v)
    out = eng.sample(x.repeat(r, 1, 1, 1).cuda().contiguous(), masks.unsqueeze(1).cuda().contiguous())
    torch.cuda.synchronize()
    assert_guards(eng, cfg.get('name'))
    return out.cpu()


def _assert_every_step_thresholds_equal(cfg, sd, x, trace, want_prob, gemm):
    thr = cfg.get('threshold', 0.5)
    for s, t in enumerate(trace):
        out = _step_probs(cfg, sd, x, t['mask_in'], s, gemm)
        assert out.shape == want_prob[s].shape
        assert max_rel(out, want_prob[s]) < REL, (cfg['name'], gemm, s)
        assert torch.equal(out > thr, want_prob[s] > thr), f'{cfg["name"]}[{gemm}]: thresholded maps of step {s} differ'


@pytest.mark.parametrize('gemm', ['bf16x3', 'f32'])
@pytest.mark.parametrize('name', U.sampler_cases())
def test_every_step_thresholded_maps_equal_the_reference(name, gemm):
    """The thresholded maps are what the x0 feedback is made of.  Every step of every fixture, r > 1 included, as single-step runs
    from the noisy maps that enter the step (the restatement's, which follow the reference's to 2e-5): with every reference
    probability >= 1e-3 off the threshold, the maps must be the REFERENCE's, pixel for pixel."""
    cfg, sd, x, noise, g = U.load(name)
    assert float(g['thr_margin']) >= 1e-3
    trace = []
    with torch.no_grad():
        U.sample(x, noise, sd, cfg, trace)
    _assert_every_step_thresholds_equal(cfg, sd, x, trace, g['prob_steps'], gemm)


def _plugin(cfg, sd):
    head = BEVDeformableHeadWithTime(**U.head_kwargs(cfg))
    head.load_state_dict({k[len('decode_head.'):]: v for k, v in sd.items() if k.startswith('decode_head.')}, strict=True)
    model = BEVDDP(bit_scale=cfg.get('bit_scale', 0.01), timesteps=cfg.get('timesteps', 1), randsteps=cfg.get('randsteps', 1),
                   feat_channels=cfg.get('feat_channels', 256))
    model.load_state_dict({k: v for k, v in sd.items() if not k.startswith('decode_head.')}, strict=True)
    return model.cuda().eval(), head.cuda().eval()


@pytest.mark.parametrize('name', U.sampler_cases())
def test_plugin_sampler_matches_reference(name):
    """the drop-in classes built with the reference's constructor arguments: both settings reach the engine"""
    cfg, sd, x, noise, g = U.load(name)
    model, head = _plugin(cfg, sd)
    out = model.ddim_sample([x.cuda()], head, noise=noise.unsqueeze(0).cuda())
    assert max_rel(out.cpu(), g['out']) < REL, name


@pytest.mark.parametrize('gemm', ['bf16x3', 'f32'])
def test_head_forward_matches_reference(gemm):
    cfg, sd, feat, _, g = U.load('head_forward')
    _, head = _plugin(cfg, sd)
    eng = guard(DDPEngine(head._state_for_engine(), 'bev', h=cfg['h'], w=cfg['w'], batch=cfg['R'], timesteps=1, gemm=gemm,
                          **head._engine_kwargs()))
    out = eng.head_forward(feat.cuda().contiguous(), g['temb'].cuda())
    torch.cuda.synchronize()
    assert_guards(eng, 'head_forward')
    assert out.shape == g['out'].shape
    assert max_rel(out.cpu(), g['out']) < REL, gemm
    if gemm == 'bf16x3':        # the module's own forward (the plugin surface of the head)
        assert max_rel(head([feat.cuda()], g['temb'].cuda()).cpu(), g['out']) < REL


def test_head_forward_with_prescale_matches_restatement():
    cfg = U.case('hf_prescale', prescale_factor=1.5, h=13, w=9, seg_conv_kernel=3)
    sd = U.state_dict_of(cfg)
    feat, _ = synthetic.make_inputs(2, 13, 9, 1, 256, 256, seed=cfg['seed'])
    from oracle import ddp_oracle as O
    temb = O.time_mlp(torch.tensor([0.3]), sd)
    _, head = _plugin(cfg, sd)
    out = head([feat.cuda()], temb.cuda()).cpu()
    with torch.no_grad():
        ref = U.head_forward(feat, temb, sd, cfg)
    assert max_rel(out, ref) < REL


# ---- oracle-driven cases beyond the fixtures (tests/bev_head_util.py: ORACLE_CASES, oracle) ----------------------------------------
@pytest.mark.parametrize('gemm', ['bf16x3', 'f32'])
@pytest.mark.parametrize('name', sorted(U.ORACLE_CASES))
def test_every_step_thresholded_maps_equal_the_restatement(name, gemm):
    """as test_every_step_thresholded_maps_equal_the_reference, on the cases beyond the fixtures: every step, every noise replica,
    torch.equal against the restatement's thresholded maps (seeds chosen by the generator's margin rule)"""
    c = U.ORACLE_CASES[name]
    sd, x, _, _ = U.oracle(c)
    trace = U.ORACLE_REF[(name, 1)][4]
    _assert_every_step_thresholds_equal(c, sd, x, trace, [t['prob'] for t in trace], gemm)


def _oracle_variants(c):
    v = ['bf16x3', 'f32', 'unfused_layer']
    if c.get('num_classes', 6) <= 8:
        v.append('unfused_tail')
    return v


@pytest.mark.parametrize('name,variant', [(n, v) for n, c in U.ORACLE_CASES.items() for v in _oracle_variants(c)])
def test_case_matches_restatement(name, variant):
    c = U.ORACLE_CASES[name]
    sd, x, noise, ref = U.oracle(c)
    gemm, flags = VARIANTS[variant]
    out = _sample(c, sd, x, noise, gemm, **flags)
    assert out.shape == ref.shape and torch.isfinite(out).all()
    err = max_rel(out, ref)
    agree = float(((out > 0.5) == (ref > 0.5)).float().mean())
    print(f'BEV-HEAD oracle {name}[{variant}]: max-rel {err:.3e} (bar {REL:.0e}), decisions equal {agree:.4f}')
    assert err < REL and agree > 0.999


@pytest.mark.parametrize('name', ['seg3_kc6', 'seg3_kc9', 'prescale_3', 'one_row'])
def test_batch_of_two_equals_two_independent_runs(name):
    c = U.ORACLE_CASES[name]
    sd, x, noise, ref = U.oracle(c, B=2)
    out = _sample(c, sd, x, noise)
    assert max_rel(out, ref) < REL
    for b in range(2):
        ob = _sample(c, sd, x[b:b + 1].clone(), noise[b:b + 1].clone())
        assert torch.equal(ob[0], out[b]), f'{name}: image {b} differs between the batched and the single-image call'


@pytest.mark.parametrize('name', ['seg3_kc6', 'seg3_kc9', 'prescale_05', 'one_row'])
def test_graph_replay_is_bit_identical(name):
    c = U.ORACLE_CASES[name]
    sd, x, noise, _ = U.oracle(c)
    eng = _engine(c, sd)
    xb, nb = x.cuda().contiguous(), noise.cuda().contiguous()
    out = eng.sample(xb, nb).clone()
    g = eng.capture(xb, nb)
    rep = g.replay().clone()
    torch.cuda.synchronize()
    assert_guards(eng, name)
    assert torch.equal(rep, out)


def test_packed_weights_of_the_wrong_kernel_are_refused():
    """a pre-packed 1x1 conv_seg with bev_seg_kernel = 3 (the library would read 9x the tensor) and the other way round"""
    from ddp_amd.engine import PackedWeights
    c = U.ORACLE_CASES['seg3_kc6']
    for packed_k, asked_k in ((1, 3), (3, 1)):
        sd = U.state_dict_of(dict(c, seg_conv_kernel=packed_k))
        pw = PackedWeights(sd, 'bev', c['num_layers'], torch.device('cuda:0'))
        with pytest.raises(ValueError, match='conv_seg.weight'):
            DDPEngine(sd, 'bev', weights=pw, **U.engine_kwargs(dict(c, seg_conv_kernel=asked_k)))


def test_one_sampler_with_two_heads_that_differ_in_prescale_only():
    """the sampler's engine cache is keyed by the head's settings: the same DDP with a second head that shares every parameter
    and differs in prescale_factor only must not reuse the first head's engine"""
    cfg, sd, x, noise, g = U.load('prescale_2')
    model, head = _plugin(cfg, sd)
    _, plain = _plugin(dict(cfg, prescale_factor=1), sd)
    nz = noise.unsqueeze(0).cuda()
    a = model.ddim_sample([x.cuda()], head, noise=nz).cpu()
    b = model.ddim_sample([x.cuda()], plain, noise=nz).cpu()
    assert max_rel(a, g['out']) < REL
    with torch.no_grad():
        ref_b = U.sample(x, noise, sd, dict(cfg, prescale_factor=1))[0]
    assert max_rel(b, ref_b) < REL and max_rel(a, b) > 100 * REL


def test_chain_and_separate_kernels_agree_with_the_3x3_head():
    """the u chain around the 3x3 head against DDP_FLAG_UNFUSED_TAIL's launches: the same operators regrouped (the bar of
    tests/config_space_cases.py for that pair, 5e-5)"""
    c = U.ORACLE_CASES['seg3_kc8']
    sd, x, noise, _ = U.oracle(c)
    a, b = _sample(c, sd, x, noise), _sample(c, sd, x, noise, fused_tail=False)
    assert max_rel(a, b) < 5e-5


# ---- routes, from the library's launch records ----------------------------------------------------------------------------------
def _expected(route, K, L):
    """tags as tests/test_config_space_gpu.py::_expected: 1 x-projection / concat-conv GEMM, 3 layer-0 projection kernel, 7 a plain
    layer kernel, 8 head launches (and the u_0 GEMM of the chain), 10 last layer + tail (k_layer MODE 8).  The 3x3 head records TWO
    tag-8 launches per step: the implicit 3x3 GEMM and k_bev_seg3."""
    return {'chain': {1: 1, 2: 0, 3: K, 7: K * (L - 1), 8: 1, 10: K},                       # 1x1 head (with or without prescale)
            'chain_seg3': {1: 1, 2: 0, 3: K, 7: K * L, 8: 1 + 2 * K, 10: 0},
            'separate': {1: 1 + K, 2: 0, 3: K, 7: K * L, 8: K, 10: 0},
            'separate_seg3': {1: 1 + K, 2: 0, 3: K, 7: K * L, 8: 2 * K, 10: 0}}[route]


@pytest.mark.parametrize('name,flags,route', [
    ('seg3_kc1', {}, 'chain_seg3'), ('seg3_kc6', {}, 'chain_seg3'), ('seg3_kc8', {}, 'chain_seg3'), ('one_row', {}, 'chain_seg3'),
    ('seg3_kc9', {}, 'separate_seg3'), ('seg3_kc32', {}, 'separate_seg3'), ('seg3_kc6', dict(fused_tail=False), 'separate_seg3'),
    ('prescale_05', {}, 'chain'), ('prescale_3', {}, 'chain'), ('prescale_2_kc9', {}, 'separate'),
    ('prescale_05', dict(fused_tail=False), 'separate')])
def test_route_witness(name, flags, route):
    """k_bev_seg3 present and MODE 8 absent with the 3x3 head; MODE 8 present without it"""
    c = U.ORACLE_CASES[name]
    sd, x, noise, _ = U.oracle(c)
    eng = _engine(c, sd, **flags)
    got = launch_counts(eng, x.cuda().contiguous(), noise.cuda().contiguous())
    assert_guards(eng, name)
    want = _expected(route, c['timesteps'], c['num_layers'])
    print(f'BEV-HEAD witness {name} ({route}): {got}')
    assert {t: got[t] for t in want} == want, (route, got)


def test_f32_engine_runs_seg3_once_per_step():
    c = U.ORACLE_CASES['seg3_kc6']
    sd, x, noise, _ = U.oracle(c)
    got = launch_counts(_engine(c, sd, 'f32'), x.cuda().contiguous(), noise.cuda().contiguous())
    assert got[10] == 0 and got[2] == 0 and got[8] == c['timesteps'], got     # (the nine shifted GEMMs carry no tag; k_bev_seg3 does)


def test_plain_configs_launch_what_they_launched():
    """a 1x1 head without prescale: the launch records of the u chain and of the separate kernels, as before ABI 7"""
    for kc, route in ((6, 'chain'), (9, 'separate')):
        c = U.case(f'plain_kc{kc}', num_classes=kc)
        sd, x, noise, _ = U.oracle(c)
        got = launch_counts(_engine(c, sd), x.cuda().contiguous(), noise.cuda().contiguous())
        want = _expected(route, c['timesteps'], c['num_layers'])
        assert {t: got[t] for t in want} == want, (route, got)
