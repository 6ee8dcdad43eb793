"""Binned depth head (``classify=True``) and the split depth range on the MI355X: ``ddp_sample`` and the stand-alone head call
against the fixtures the reference made (tests/golden/depth_bins/) under both engines, the plugin path end to end, batches,
hipGraph replay, and one C4-size map against the CPU restatement."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ddp_amd  # noqa: E402
from ddp_amd.engine import DDPEngine  # noqa: E402
from ddp_amd.utils import synthetic  # noqa: E402
import depth_bins_util as U  # noqa: E402
from golden_util import max_rel  # noqa: E402
from support import REL  # noqa: E402  (the depth bar of test_hip_parity.py)

pytestmark = pytest.mark.gpu


def _engine_kwargs(cfg):
    head = U.head_of(cfg)
    kw = dict(timesteps=cfg.get('timesteps', 1), randsteps=cfg.get('randsteps', 1), bit_scale=cfg.get('bit_scale', 0.1),
              time_difference=cfg.get('time_difference', 1), min_depth=cfg['min_depth'], max_depth=cfg['max_depth'],
              head_min_depth=head['min_depth'], head_max_depth=head['max_depth'], depth_scale_up=head['scale_up'],
              depth_use_eps=head['use_eps'])
    if head['classify']:
        kw.update(depth_bins=U.bins_of(head), depth_norm=head['norm_strategy'])
    return kw


def _model(cfg, sd):
    m = ddp_amd.build_depther(U.depther_cfg(cfg))
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


@pytest.mark.parametrize('gemm', ['bf16x3', 'f32'])
@pytest.mark.parametrize('name', U.sampler_cases())
def test_ddp_sample_matches_reference(name, gemm):
    cfg, sd, x, noise, g = U.load(name)
    eng = DDPEngine(sd, 'depth', h=cfg['h'], w=cfg['w'], gemm=gemm, **_engine_kwargs(cfg))
    out = eng.sample(x.cuda(), noise.unsqueeze(0).cuda().contiguous())
    torch.cuda.synchronize()
    assert out.shape == g['out'].shape
    assert max_rel(out.cpu(), g['out']) < REL, (name, gemm)


@pytest.mark.parametrize('variant', [dict(fused_layer=False), dict(fused_prologue=False), dict(fused_tail=False),
                                     dict(nchw_head=False)], ids=['unfused_layer', 'unfused_prologue', 'unfused_tail', 'sb_head'])
@pytest.mark.parametrize('name', ['ud_softmax_r2', 'ud_sigmoid_td2', 'range_split_scale_up'])
def test_ddp_sample_diagnostic_variants(name, variant):
    """the binned head and the split range behind the diagnostic switches of the bf16x3 engine (the tile-GEMM layers leave their
    output as SB only: the binned head converts it for the stream GEMM)"""
    cfg, sd, x, noise, g = U.load(name)
    eng = DDPEngine(sd, 'depth', h=cfg['h'], w=cfg['w'], gemm='bf16x3', **variant, **_engine_kwargs(cfg))
    out = eng.sample(x.cuda(), noise.unsqueeze(0).cuda().contiguous())
    assert max_rel(out.cpu(), g['out']) < REL, (name, variant)


@pytest.mark.parametrize('name', U.sampler_cases())
def test_plugin_sampler_matches_reference(name):
    """the drop-in depther built from the config dict: both depth ranges and the bins reach the engine"""
    cfg, sd, x, noise, g = U.load(name)
    model = _model(cfg, sd)
    out = model.sample(x.cuda(), None, noise=noise.unsqueeze(0).cuda())
    assert max_rel(out.cpu(), g['out']) < REL, name


@pytest.mark.parametrize('gemm', ['bf16x3', 'f32'])
def test_head_forward_matches_reference_trace(gemm):
    cfg, sd, feat, _, g = U.load('head_forward')
    head = U.head_of(cfg)
    hsd = {k[len('decode_head.'):]: v for k, v in sd.items() if k.startswith('decode_head.')}
    m = ddp_amd.build_depther(U.depther_cfg(cfg)).decode_head
    m.load_state_dict(hsd, strict=True)
    m = m.cuda().eval()
    eng = DDPEngine(m._state_for_engine(), 'depth', h=cfg['h'], w=cfg['w'], batch=cfg['R'], timesteps=1, gemm=gemm,
                    min_depth=head['min_depth'], max_depth=head['max_depth'], depth_bins=m.depth_bins(),
                    depth_norm=head['norm_strategy'])
    out = eng.head_forward(feat.cuda().contiguous(), g['temb'].cuda())
    assert out.shape == g['out'].shape
    assert max_rel(out.cpu(), g['out']) < REL, gemm
    # the module's own forward (the plugin surface of the head)
    out2 = m([feat.cuda()], g['temb'].cuda())
    assert max_rel(out2.cpu(), g['out']) < REL


@pytest.mark.parametrize('name', ['ud_softmax_r2', 'range_split'])
def test_harness_call_end_to_end(name):
    """``model(return_loss=False, **data)`` (depth/depth/apis/test.py:88): sampler with its own noise, clamp to the HEAD's range,
    resize to the input - against the CPU restatement of the sampler and the oracle's epilogue."""
    from oracle import ddp_oracle as O
    cfg, sd, x, _, _ = U.load(name)
    model = _model(cfg, sd)
    h, w, r = cfg['h'], cfg['w'], cfg['randsteps']
    H, W = 4 * h, 4 * w
    model.extract_feat = lambda img: [x.cuda()]
    meta = dict(img_shape=(H, W, 3), ori_shape=(H, W, 3), pad_shape=(H, W, 3), flip=False)
    torch.manual_seed(11)
    res = model(return_loss=False, img=[torch.zeros(1, 3, H, W, device='cuda')], img_metas=[[meta]])
    torch.manual_seed(11)
    noise = torch.randn((1, r, 1, h, w), device='cuda').cpu()
    head = U.head_of(cfg)
    with torch.no_grad():
        ref = O.depth_postprocess([U.sample(x, noise[0], sd, cfg)], [None], (H, W), head['min_depth'], head['max_depth'])
    assert len(res) == 1 and res[0].shape == (1, H, W)
    assert max_rel(torch.from_numpy(res[0]), ref[0]) < REL


def test_batch_equals_independent_runs_and_graph_replay():
    cfg, sd, _, _, _ = U.load('ud_softmax_r2')
    B, h, w, r = 3, cfg['h'], cfg['w'], cfg['randsteps']
    xs, ns = synthetic.make_inputs(B, h, w, r, 256, 1, seed=77)
    kw = _engine_kwargs(cfg)
    eng = DDPEngine(sd, 'depth', h=h, w=w, batch=B, **kw)
    xb, nb = xs.cuda().contiguous(), ns.cuda().contiguous()
    out = eng.sample(xb, nb).clone()
    one = DDPEngine(sd, 'depth', h=h, w=w, batch=1, **kw)
    for i in range(B):
        oi = one.sample(xb[i:i + 1].clone(), nb[i:i + 1].clone())      # (fresh, aligned buffers)
        assert torch.equal(oi, out[i:i + 1]), i
    g = eng.capture(xb, nb)
    rep = g.replay().clone()
    torch.cuda.synchronize()
    assert torch.equal(rep, out)


def test_c4_size_binned_map_matches_cpu_restatement():
    """one KITTI C4-size feature map (88 x 304), 256 bins, linear normalisation"""
    cfg = dict(min_depth=1e-3, max_depth=80.0, bit_scale=0.1, timesteps=1, randsteps=1, time_difference=1, h=88, w=304,
               head=dict(classify=True, n_bins=256, bins_strategy='UD', norm_strategy='linear'))
    sd = synthetic.make_state_dict('depth', 1, 6, 256, seed=500, n_bins=256)
    x, noise = synthetic.make_inputs(1, 88, 304, 1, 256, 1, seed=501)
    eng = DDPEngine(sd, 'depth', h=88, w=304, **_engine_kwargs(cfg))
    out = eng.sample(x.cuda(), noise.cuda().contiguous()).cpu()
    torch.set_num_threads(16)
    with torch.no_grad():
        ref = U.sample(x, noise[0], sd, cfg)
    assert torch.isfinite(out).all()
    assert max_rel(out, ref) < REL
