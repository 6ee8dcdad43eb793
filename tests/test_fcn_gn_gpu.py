"""GroupNorm convolutions of FCNHeadWithTime on the GPU (cases and expectation: tests/fcn_gn_cases.py; their CPU companion:
tests/test_fcn_gn_host.py).  ``ddp_fcn_head_forward`` and ``ddp_sample_fcn`` through the C ABI on guarded, exactly sized workspaces
(as tests/test_next_rows_gpu.py), through the plugin class and the segmentor; against the fp32 expectation and the fixtures made by
the reference class at the project's REL = 2e-4 (max_rel).  Every GroupNorm case fails on the parent commit with DDP_E_NULL
("incomplete norm"), the plugin tests with NotImplementedError.  The BatchNorm / norm-free paths: same bits as the parent's build."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import fcn_gn_cases as G
from ddp_amd import _lib
from golden_util import max_rel
from support import REL, FixedBackbone as _Backbone, Guarded, assert_guards as _assert_guards, dev, finite as _finite, stream as _stream  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bar_is_the_suite_bar():
    assert G.REL == REL == 2e-4


def _run_head(c, sd, dev, feat, temb, what=''):
    """ddp_fcn_head_forward through the C ABI, the conv array straight from the state dict, on a guarded workspace"""
    lib = _lib.load()
    maps = feat.shape[0]
    g = Guarded(G.head_query(lib, c, maps), dev)
    arr, keep = G.conv_array(sd, c, dev)
    wseg = sd['conv_seg.weight'].reshape(c['classes'], 256).contiguous().to(dev)
    bseg = sd['conv_seg.bias'].contiguous().to(dev)
    out = torch.full((maps, c['classes'], c['h'], c['w']), float('nan'), device=dev)
    _lib.check(lib.ddp_fcn_head_forward(arr, c['num_convs'], c['dilation'], wseg.data_ptr(), bseg.data_ptr(), c['classes'], feat.data_ptr(),
                                        temb.data_ptr() if temb is not None else None, maps, c['h'], c['w'], out.data_ptr(), g.ptr(),
                                        _stream(dev)), lib)
    torch.cuda.synchronize()
    _assert_guards(g, f'fcn_gn {c["name"]} {what}')
    _finite(out, f'fcn_gn {c["name"]} {what}')
    return out


def _plugin_head(c, sd, dev, concat_input=False):
    import ddp_amd
    norm = dict(type='GN', num_groups=32) if c['eps'] == 1e-5 else dict(type='GN', num_groups=32, eps=c['eps'])
    head = ddp_amd.FCNHeadWithTime(num_convs=c['num_convs'], kernel_size=3, concat_input=concat_input, dilation=c['dilation'],
                                   in_channels=256, channels=256, num_classes=c['classes'], in_index=0, norm_cfg=norm)
    head.load_state_dict(sd, strict=True)
    return head.to(dev).eval()


def _uniform_gn(c):
    return all(k == 'gn' for k in c['norms']) and not c['conv_b']


@pytest.mark.parametrize('name', list(G.HEAD))
def test_head_matches_expectation(dev, name):
    """C ABI against the fp32 expectation (< REL); a second call and, where the plugin class can hold the case (one norm for the whole
    head, no conv bias), the plugin class give the same bits; every map of a batched call equals its single-map call bit for bit
    (the statistics are per map)."""
    c = G.HEAD[name]
    sd = G.head_state(c)
    feat, temb = G.head_inputs(c)
    feat = feat.to(dev)
    temb = temb[0].contiguous().to(dev) if temb is not None else None
    out = _run_head(c, sd, dev, feat, temb)
    ref = G.head_expect(c)
    err = max_rel(out.cpu(), ref)
    print(f'FCN-GN head {name}: max-rel {err:.3e} (bar {REL:.0e}), {"fused" if G.fused_route(c) else "stand-alone"} statistics')
    assert out.shape == ref.shape and err < REL
    assert torch.equal(out, _run_head(c, sd, dev, feat, temb, what='second call'))
    if _uniform_gn(c):
        head = _plugin_head(c, sd, dev)
        assert torch.equal(head([feat], temb[None] if temb is not None else None), out), f'{name}: plugin class and C ABI differ'
    if c['maps'] > 1:
        for b in range(c['maps']):
            one = _run_head(c, sd, dev, feat[b:b + 1].contiguous(), temb, what=f'map {b} alone')
            assert torch.equal(one[0], out[b]), f'{name}: map {b} differs between the batched and the single call'


@pytest.mark.parametrize('name', G.FIXTURE_HEADS)
def test_head_matches_reference_fixture(dev, name):
    """the reference class's own output (tests/golden/fcn_gn/, gen_fcn_gn_golden.py): C ABI and plugin class < REL"""
    c, feat, temb, sd, ref = G.load_fixture_head(name)
    feat = feat.to(dev)
    t1 = temb[0].contiguous().to(dev) if temb is not None else None
    out = _run_head(c, sd, dev, feat, t1)
    head = _plugin_head(c, sd, dev, concat_input=c['concat_input'])
    via_plugin = head([feat], temb.expand(c['maps'], 1024).to(dev) if temb is not None else None)
    e1, e2 = max_rel(out.cpu(), ref), max_rel(via_plugin.cpu(), ref)
    print(f'FCN-GN fixture {name}: max-rel C ABI {e1:.3e}, plugin {e2:.3e} (bar {REL:.0e})')
    assert e1 < REL and e2 < REL and torch.equal(out, via_plugin)


# ---- the sampler loop ----------------------------------------------------------------------------------------------------------
def _loop_checks(c, sd, dev, x, noise, sn, ref, decisions):
    x, noise, sn = [t.contiguous().to(dev) if t is not None else None for t in (x, noise, sn)]
    out = G.device_loop(c, sd, dev).sample(x, noise, sn, what='self-preparing')
    o = out.cpu()
    errs = [max_rel(o[b:b + 1], ref[b:b + 1]) for b in range(c['B'])]
    print(f'FCN-GN loop {c["name"]}: max-rel per image {" ".join(f"{e:.3e}" for e in errs)} (bar {REL:.0e})')
    assert out.shape == ref.shape and max(errs) < REL
    prepared = G.device_loop(c, sd, dev)
    prepared.prepare()
    assert torch.equal(prepared.sample(x, noise, sn, what='prepared'), out), 'prepared and self-preparing calls differ'
    assert torch.equal(prepared.sample(x, noise, sn, what='prepared, second call'), out)
    rec = G.device_loop(c, sd, dev, flags=_lib.FLAG_STEP_RECORD)
    assert torch.equal(rec.sample(x, noise, sn, what='step record'), out), 'DDP_FLAG_STEP_RECORD changed the output'
    got = rec.record()
    if decisions is not None:
        assert got.shape == decisions.shape and torch.equal(got, decisions), \
            f'{int((got != decisions).sum())} of {decisions.numel()} recorded decisions differ from the expectation\'s'
    if c['B'] > 1:
        one = G.device_loop(c, sd, dev, batch=1)
        for b in range(c['B']):
            ob = one.sample(x[b:b + 1].contiguous(), noise[b:b + 1].contiguous(), sn[:, b:b + 1].contiguous() if sn is not None else None,
                            what=f'image {b} alone')
            assert torch.equal(ob[0], out[b]), f'image {b} differs between the batched and the single-image call'
    return out


@pytest.mark.parametrize('name', list(G.LOOP))
def test_loop_matches_expectation(dev, name):
    """ddp_sample_fcn (ddim and ddpm cases; B * r of 1, 2, 2 x 2; one case with a BatchNorm conv beside the GroupNorm conv): output
    < REL per image; with and without DDP_FLAG_FCN_PREPARED bit-identical; with DDP_FLAG_STEP_RECORD the same output and, at every
    step, exactly the expectation's decisions (the fp64 expectation keeps a top-2 margin of 1e-3, test_fcn_gn_host.py); the batched
    call gives the bits of single-image calls."""
    c = G.LOOP[name]
    ref, steps = G.loop_expect(c)
    _loop_checks(c, G.loop_state(c), dev, *G.loop_inputs(c), ref, G.loop_decisions(steps))


@pytest.mark.parametrize('name', G.FIXTURE_LOOPS)
def test_loop_matches_reference_fixture(dev, name):
    """the reference's ddim_sample / ddpm_sample around the reference's GroupNorm head (tests/golden/fcn_gn/): < REL.  The decisions
    are compared where the reference's own top-2 margin is at least MARGIN of the step's largest |score| (these maps are too large
    for a seed that keeps the margin everywhere: smallest 6.5e-5 and 5.1e-4)."""
    c, sd, x, noise, sn, ref, logits = G.load_fixture_loop(name)
    out = _loop_checks(c, sd, dev, x, noise, sn, ref, None)
    rec = G.device_loop(c, sd, dev, flags=_lib.FLAG_STEP_RECORD)
    rec.sample(x.to(dev), noise.contiguous().to(dev), sn.contiguous().to(dev) if sn is not None else None, what='step record')
    got = rec.record()[:, 0]                                                         # (K, r, h, w)
    t = logits.topk(2, dim=2).values
    safe = (t[:, :, 0] - t[:, :, 1]) >= G.MARGIN * logits.abs().amax(dim=(1, 2, 3, 4), keepdim=True)[:, :, 0]
    want = logits.argmax(2).to(torch.uint8)
    assert safe.float().mean() > 0.9 and torch.equal(got[safe], want[safe])
    assert float((out.cpu().argmax(1) == ref.argmax(1)).float().mean()) > 0.999


def _segmentor(c, sd, dev, **kw):
    import ddp_amd
    norm = dict(type='GN', num_groups=32) if c['eps'] == 1e-5 else dict(type='GN', num_groups=32, eps=c['eps'])
    model = ddp_amd.build_segmentor(dict(
        type='DDP', timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'], accumulation=c['accumulation'], diffusion=c['sampler'],
        decode_head=dict(type='FCNHeadWithTime', num_convs=c['num_convs'], concat_input=False, dilation=c['dilation'], in_channels=256,
                         channels=256, num_classes=c['classes'], in_index=0, norm_cfg=norm), **kw))
    model.load_state_dict(sd, strict=True)
    return model.to(dev).eval()


@pytest.mark.parametrize('name', ['b1_ddim_fused', 'b2_ddpm_odd', 'b2_r2_ddim'])
def test_segmentor_with_gn_head(dev, name):
    """the seg ``DDP`` segmentor with ``norm_cfg=dict(type='GN', num_groups=32)`` in its FCN decode head: ddim_sample / ddpm_sample
    (FcnSamplerEngine) give the bits of the C ABI call; simple_test runs end to end and labels as the argmax of the resized scores."""
    c = G.LOOP[name]
    sd = G.loop_state(c)
    x, noise, sn = [t.to(dev) if t is not None else None for t in G.loop_inputs(c)]
    model = _segmentor(c, sd, dev)
    out = model.ddpm_sample(x, noise=noise, step_noise=sn) if c['sampler'] == 'ddpm' else model.ddim_sample(x, noise=noise)
    assert torch.equal(out, G.device_loop(c, sd, dev).sample(x, noise, sn, what='beside the segmentor'))
    assert max_rel(out.cpu(), G.loop_expect(c)[0]) < REL
    model.backbone = _Backbone(x)
    H, W = c['h'] * 4, c['w'] * 4
    img = torch.zeros(c['B'], 3, H, W, device=dev)
    torch.manual_seed(5)
    drawn = torch.randn((c['B'], c['r'], 256, c['h'], c['w']), device=dev)
    dsn = torch.randn((c['K'], c['B'], c['r'], 256, c['h'], c['w']), device=dev) if c['sampler'] == 'ddpm' else None
    scores = model.ddpm_sample(x, noise=drawn, step_noise=dsn) if dsn is not None else model.ddim_sample(x, noise=drawn)
    ref = F.interpolate(scores, size=(H, W), mode='bilinear', align_corners=False).argmax(1).cpu()
    torch.manual_seed(5)
    lab = torch.from_numpy(__import__('numpy').stack(model.simple_test(img, None, rescale=False)))
    assert lab.shape == ref.shape and float((lab != ref).float().mean()) < 1e-3


@pytest.mark.parametrize('name', ['b1_ddim_fused', 'b2_ddpm_odd'])
def test_seeded_noise_with_gn_head(dev, name):
    """DDP_FLAG_SEEDED_NOISE through FcnSamplerEngine: the same seed gives the same bits, another seed another map; ddim: feeding the
    start noise the device generated to an unseeded engine gives the seeded call's bits."""
    from ddp_amd.engine import FcnSamplerEngine
    c = G.LOOP[name]
    sd = G.loop_state(c)
    x = G.loop_inputs(c)[0].to(dev)
    head = _plugin_head(c, {k[len('decode_head.'):]: v for k, v in sd.items() if k.startswith('decode_head.')}, dev)
    kw = dict(h=c['h'], w=c['w'], batch=c['B'], randsteps=c['r'], timesteps=c['K'], num_classes=c['classes'], bit_scale=c['bit_scale'],
              sampler=c['sampler'], accumulation=c['accumulation'], device=dev)
    eng = FcnSamplerEngine(sd, head, seeded_noise=True, **kw)
    a = eng.sample(x, seed=1234).clone()
    noise = eng.last_noise().clone()
    assert torch.isfinite(a).all() and torch.equal(eng.sample(x, seed=1234), a)
    assert not torch.equal(eng.sample(x, seed=1235), a)
    if c['sampler'] == 'ddim':
        assert torch.equal(FcnSamplerEngine(sd, head, **kw).sample(x, noise=noise), a)


def test_incomplete_norms_stay_refused(dev):
    """every partial combination but (bn_w, bn_b, NULL, NULL) keeps the parent's answer: DDP_E_NULL, 'incomplete norm'"""
    c = G.HEAD['wave_4x8']
    sd = G.head_state(c)
    feat = G.head_inputs(c)[0].to(dev)
    lib = _lib.load()
    arr, keep = G.conv_array(sd, c, dev)
    spare = torch.ones(256, device=dev)
    ws = torch.empty(G.head_query(lib, c) // 4, device=dev)
    wseg = sd['conv_seg.weight'].reshape(c['classes'], 256).contiguous().to(dev)
    out = torch.empty((c['maps'], c['classes'], c['h'], c['w']), device=dev)
    gamma, beta = arr[0].bn_w, arr[0].bn_b
    for w_, b_, m_, v_ in [(gamma, beta, spare.data_ptr(), None), (gamma, beta, None, spare.data_ptr()), (gamma, None, None, None),
                           (gamma, None, spare.data_ptr(), spare.data_ptr())]:
        arr[0].bn_w, arr[0].bn_b, arr[0].bn_mean, arr[0].bn_var = w_, b_, m_, v_
        rc = lib.ddp_fcn_head_forward(arr, c['num_convs'], c['dilation'], wseg.data_ptr(), None, c['classes'], feat.data_ptr(), None,
                                      c['maps'], c['h'], c['w'], out.data_ptr(), ws.data_ptr(), _stream(dev))
        assert rc != 0 and b'incomplete norm' in lib.ddp_last_error()
    torch.cuda.synchronize()


def test_bn_and_norm_free_paths_give_the_parents_bits(dev):
    """tests/golden/fcn_gn/parent_bits.json: sha256 of the outputs of the BatchNorm / norm-free heads on the existing fcn_* and
    loopfcn_* fixtures, recorded from a library built from the parent commit (tests/golden/gen_fcn_gn_parent.py bits)"""
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'fcn_gn', 'parent_bits.json')))
    got = G.unchanged_path_hashes(dev)
    assert len(want) >= 6 and got == want
