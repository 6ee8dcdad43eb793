"""Every sampler path and configuration limit against the CPU oracle.  Needs an MI355X: ``pytest -m gpu``.

``ddp_sample`` picks its kernels from the configuration; the reference-made fixtures reach a few regions of that space only.
The cases of tests/config_space_cases.py cover the rest - BEV with 1 .. 32 classes (the u chain up to 8, the separate kernels
above), feature widths other than 256, one-row / one-column / one-pixel depth maps and L = 1, DDP_MAX_LAYERS and DDP_MAX_STEPS,
DDPM with B > 1 and r > 1 - each on both engines and under every diagnostic flag that selects another route for it, each image
of a batched call against its own run of ``oracle.ddp_oracle`` in fp32 at the bar of tests/test_hip_parity.py (REL = 2e-4;
tests/test_config_space_host.py shows on the CPU that the oracle is conditioned well enough on every case for that bar).

Every engine of this file samples through a workspace that starts and ends with a 4 KiB guard and is filled with a NaN
pattern, interior included: the guards must come back untouched (the sizing arithmetic of ``carve()``), and a kernel that reads
workspace bytes nobody wrote shows as a NaN in the output.

The route a case takes is read from the library's own launch records (``ddp_profile_begin(255)``), see
``test_path_witness``."""
import pytest
import torch

import config_space_cases as S
import support
from ddp_amd import _lib
from golden_util import max_rel
from support import REL, assert_guards, dev, launch_counts  # noqa: F401

pytestmark = pytest.mark.gpu

VARIANTS = {(n, vid): (gemm, flags) for n, c in S.CASES.items() for vid, gemm, flags in S.variants(c)}
_OUT = {}
_state = support.state_cache(S.state_dict, S.inputs)


def _engine(c, dev, gemm='bf16x3', **flags):
    """DDPEngine of the case on a guarded, NaN-filled workspace; the cfg is the one the CPU companion queried"""
    eng = support.engine(_state(c)[0], c['task'], S.engine_kwargs(c), dev, gemm, **flags)
    assert S.cfg_bytes(eng.cfg) == S.cfg_bytes(S.make_cfg(c, gemm, **flags)), 'engine and config_space_cases.make_cfg disagree'
    return eng


def _sample(c, dev, gemm='bf16x3', **flags):
    _, (x, noise, sn) = _state(c)
    eng = _engine(c, dev, gemm, **flags)
    out = eng.sample(x.to(dev), noise.to(dev), sn.to(dev) if sn is not None else None)
    torch.cuda.synchronize()
    assert_guards(eng, c['name'])
    return out.cpu()


def _output(name, vid, dev):
    if (name, vid) not in _OUT:
        gemm, flags = VARIANTS[(name, vid)]
        _OUT[(name, vid)] = _sample(S.CASES[name], dev, gemm, **flags)
    return _OUT[(name, vid)]


def test_bar_is_the_suite_bar():
    assert S.REL == REL == 2e-4 and S.COND == REL / 20


@pytest.mark.parametrize('name,vid', sorted(VARIANTS))
def test_case_matches_oracle(dev, name, vid):
    """B images in one call, each against its own fp32 oracle run: max-rel < REL, argmax / > threshold agreement > 0.999;
    workspace guards untouched.  Feature-width cases: afterwards a fresh engine samples another, previously verified
    configuration (the smoke test's model at 5 x 7) - an overrun that corrupted a neighbouring allocation has a chance to show."""
    c = S.CASES[name]
    S.check_against_oracle(c, _output(name, vid, dev), f'{name}[{vid}]')
    if c['family'] == 'feature_width':
        S.check_against_oracle(S.CANARY, _sample(S.CANARY, dev, VARIANTS[(name, vid)][0]), f'canary after {name}[{vid}]')


@pytest.mark.parametrize('name', [n for n, c in S.CASES.items() if c['task'] == 'seg' and c['sampler'] == 'ddim'])
def test_seg_tail_fused_and_unfused_same_bits(dev, name):
    """include/ddp_mi355x.h:86-92: k_layer MODE 6 against MODE 0 + MODE 4 / 1 is the same arithmetic - bit-identical at every
    feature width, at 12 layers and 64 steps, with accumulation off (prob_mode 0 then 3)."""
    assert torch.equal(_output(name, 'bf16x3', dev), _output(name, 'unfused-tail', dev))


@pytest.mark.parametrize('name', [n for n, c in S.CASES.items() if c['task'] == 'bev' and c['Kc'] <= 8])
def test_bev_u_chain_and_separate_kernels_agree(dev, name):
    """the u chain (k_bev_u_update, k_bev_q, k_layer MODE 8) against DDP_FLAG_UNFUSED_TAIL's launches on the same <= 8-class
    case: the same operators regrouped - the bar of test_fused_and_unfused_step_boundary_depth_bev (5e-5), same decisions"""
    c = S.CASES[name]
    a, b = _output(name, 'bf16x3', dev), _output(name, 'unfused-tail', dev)
    err = max_rel(a, b)
    print(f'CONFIG-SPACE bev_pair {name}: u chain vs separate kernels max-rel {err:.3e} (bar {S.BEV_FUSED_UNFUSED:.0e})')
    assert err < S.BEV_FUSED_UNFUSED
    assert float(((a > c['threshold']) == (b > c['threshold'])).float().mean()) > 0.9995


# (depth_1x127_L2 is left out: its two images do not fit the chain, one image does - the batched and the single-image call run
# different step heads and agree to rounding only; both are compared with the oracle above)
@pytest.mark.parametrize('name', [n for n in S.names('depth_fallbacks') if n != 'depth_1x127_L2'] +
                         ['bev_kc1_r2', 'bev_kc8_r1', 'bev_kc9_r2', 'bev_kc32_r1', 'depth_L12_r2', 'depth_K1'])
def test_batched_call_equals_single_image_calls(dev, name):
    """The step heads index the tokens of ALL maps of a call.  On one-row, one-column and one-pixel maps, at L = 1 and r = 2
    (k_layer MODE 3 with the fused previous-step depth update: lanes past M read dvec[M - 1], which another wave updates in
    place) and in both BEV regimes, the batched call must give, image by image, the bits of single-image calls - a double
    update or a token of the neighbouring image would show here."""
    from ddp_amd.engine import DDPEngine
    c = S.CASES[name]
    sd, (x, noise, _) = _state(c)
    out = _output(name, 'bf16x3', dev)
    kw = dict(S.engine_kwargs(c), batch=1)
    one = DDPEngine(sd, c['task'], device=dev, gemm='bf16x3', **kw)
    for b in range(c['B']):
        o = one.sample(x[b:b + 1].clone().to(dev), noise[b:b + 1].clone().to(dev)).cpu()
        assert torch.equal(o[0], out[b]), f'{name}: image {b} differs between the batched and the single-image call'


@pytest.mark.parametrize('base,over,word', S.REFUSALS)
def test_limits_are_refused(dev, base, over, word):
    """33 BEV classes, 13 layers, 65 steps: DdpError from the engine's constructor, before any device work"""
    from ddp_amd.engine import DDPEngine
    c = dict(S.CASES[base], **over)
    with pytest.raises(_lib.DdpError, match=word):
        DDPEngine(S.state_dict(c), c['task'], device=dev, **S.engine_kwargs(c))


# ---- path witnesses -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n, c in S.CASES.items() if 'path' in c])
def test_path_witness(dev, name):
    """The case runs the route it was written for (bf16x3, default flags): launch counts per tag from ddp_profile_read.

    Not distinguishable by tags, so not claimed: 'depth_bins' against a regression head under DDP_FLAG_UNFUSED_TAIL (both: MODE 3
    step head, plain last layer, one tag-8 head launch per step); 'bev_separate' against a <= 8-class case under
    DDP_FLAG_UNFUSED_TAIL (the same launches by construction); head7 against the prologue path at K = 1 on tag 2 (tag 1 tells them
    apart); k_depth_head, k_bev_q, k_bev_u_update and the update kernels carry no tag.  One process-wide session: not run
    concurrently."""
    c = S.CASES[name]
    _, (x, noise, sn) = _state(c)
    eng = _engine(c, dev)
    got = launch_counts(eng, x.to(dev), noise.to(dev), sn.to(dev) if sn is not None else None)
    assert_guards(eng, name)
    want = S.expected_launches(c['path'], c['K'], c['L'])
    print(f'CONFIG-SPACE witness {name} ({c["path"]}): {got}')
    assert {t: got[t] for t in want} == want, (c['path'], got)


@pytest.mark.parametrize('name,flags,path', [
    ('bev_kc8_r1', dict(fused_tail=False), 'bev_separate'), ('bev_kc1_r2', dict(fused_prologue=False), 'bev_separate'),
    ('seg_L12', dict(fused_tail=False), 'seg_unfused_tail_head7'), ('seg_cx96_r1', dict(fused_tail=False), 'seg_unfused_tail_prologue'),
    ('seg_L12', dict(nchw_head=False), 'seg_prologue'), ('depth_cx512', dict(fused_tail=False), 'depth_unfused_tail'),
    ('depth_9x11_L1', dict(fused_tail=False), 'depth_unfused_tail')])
def test_path_witness_of_the_diagnostic_flags(dev, name, flags, path):
    """the flags do select the launches they are documented to select (otherwise the variants above would test one route twice)"""
    c = S.CASES[name]
    _, (x, noise, sn) = _state(c)
    eng = _engine(c, dev, **flags)
    got = launch_counts(eng, x.to(dev), noise.to(dev))
    want = S.expected_launches(path, c['K'], c['L'])
    assert {t: got[t] for t in want} == want, (path, got)


def test_f32_engine_runs_none_of_the_fused_kernels(dev):
    c = S.CASES['bev_kc8_r1']
    _, (x, noise, _) = _state(c)
    got = launch_counts(_engine(c, dev, 'f32'), x.to(dev), noise.to(dev))
    assert got[10] == 0 and got[2] == 0 and got[8] == c['K'], got        # (its tile GEMMs carry tags 1, 3 .. 8; no k_layer launch exists)
