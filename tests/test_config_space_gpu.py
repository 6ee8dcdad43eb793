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
import ctypes as C

import pytest
import torch

import config_space_cases as S
from ddp_amd import _lib
from golden_util import max_rel
from test_hip_parity import REL

pytestmark = pytest.mark.gpu

GUARD = 1024                 # floats: 4 KiB in front of and behind the workspace
PATTERN = 0x7FC0BEEF         # a quiet NaN with a payload nobody computes


@pytest.fixture(scope='module')
def dev():
    return torch.device('cuda:0')


def variants(c):
    """(id, gemm, flags) of the case: both engines, and every diagnostic flag that selects another route for the configuration
    (flags act on the bf16x3 engine only; include/ddp_mi355x.h:66-92)"""
    v = [('bf16x3', 'bf16x3', {}), ('f32', 'f32', {}), ('unfused-layer', 'bf16x3', dict(fused_layer=False))]
    seg_ddim = c['task'] == 'seg' and c['sampler'] == 'ddim'
    if c['task'] == 'seg' and c['sampler'] == 'ddpm':           # (no tail kernels on the DDPM path: the step prologue is the only other switch)
        v.append(('unfused-prologue', 'bf16x3', dict(fused_prologue=False)))
    if seg_ddim or (c['task'] == 'depth' and not c['n_bins']) or (c['task'] == 'bev' and c['Kc'] <= 8):
        v.append(('unfused-tail', 'bf16x3', dict(fused_tail=False)))
        v.append(('unfused-prologue', 'bf16x3', dict(fused_prologue=False)))
    if c['task'] == 'depth' and c['n_bins']:
        v.append(('unfused-prologue', 'bf16x3', dict(fused_prologue=False)))
    if seg_ddim and c['Cx'] == 256 and c['r'] == 1:
        v.append(('sb-head', 'bf16x3', dict(nchw_head=False)))
    return v


VARIANTS = {(n, vid): (gemm, flags) for n, c in S.CASES.items() for vid, gemm, flags in variants(c)}
_SD, _IN, _OUT = {}, {}, {}


def _state(c):
    if c['name'] not in _SD:
        _SD[c['name']] = S.state_dict(c)
        _IN[c['name']] = S.inputs(c)
    return _SD[c['name']], _IN[c['name']]


def _engine(c, dev, gemm='bf16x3', **flags):
    """DDPEngine of the case on a guarded, NaN-filled workspace; the cfg is the one the CPU companion queried"""
    from ddp_amd.engine import DDPEngine
    sd, _ = _state(c)
    eng = DDPEngine(sd, c['task'], device=dev, gemm=gemm, **flags, **S.engine_kwargs(c))
    assert S.cfg_bytes(eng.cfg) == S.cfg_bytes(S.make_cfg(c, gemm, **flags)), 'engine and config_space_cases.make_cfg disagree'
    n = eng.workspace.numel()                 # = ddp_query_workspace(cfg) / 4: the engine owns the allocation
    buf = torch.empty(n + 2 * GUARD, dtype=torch.float32, device=dev)
    buf.view(torch.int32).fill_(PATTERN)
    eng.guarded = buf
    eng.workspace = buf[GUARD:GUARD + n]
    assert eng.workspace.data_ptr() % 256 == 0
    return eng


def _assert_guards(eng, what):
    bits = eng.guarded.view(torch.int32)
    front, back = bits[:GUARD], bits[-GUARD:]
    bad_f, bad_b = int((front != PATTERN).sum()), int((back != PATTERN).sum())
    assert bad_f == 0 and bad_b == 0, f'{what}: {bad_f} words written in front of the workspace, {bad_b} behind it'


def _sample(c, dev, gemm='bf16x3', **flags):
    _, (x, noise, sn) = _state(c)
    eng = _engine(c, dev, gemm, **flags)
    out = eng.sample(x.to(dev), noise.to(dev), sn.to(dev) if sn is not None else None)
    torch.cuda.synchronize()
    _assert_guards(eng, c['name'])
    return out.cpu()


def _output(name, vid, dev):
    if (name, vid) not in _OUT:
        gemm, flags = VARIANTS[(name, vid)]
        _OUT[(name, vid)] = _sample(S.CASES[name], dev, gemm, **flags)
    return _OUT[(name, vid)]


def _check_against_oracle(c, out, label):
    ref = S.oracle_batch(c)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all(), f'{label}: non-finite output'
    errs = [max_rel(out[b:b + 1], ref[b:b + 1]) for b in range(c['B'])]
    d, dr = S.decisions(c, out), S.decisions(c, ref)
    agree = 1.0 if d is None else float((d == dr).float().mean())
    print(f'CONFIG-SPACE {c["family"]} {label}: max-rel per image {" ".join(f"{e:.3e}" for e in errs)} (bar {REL:.0e}), '
          f'decisions equal {agree:.4f}')
    assert max(errs) < REL and agree > 0.999
    return max(errs)


def test_bar_is_the_suite_bar():
    assert S.REL == REL == 2e-4 and S.COND == REL / 20


@pytest.mark.parametrize('name,vid', sorted(VARIANTS))
def test_case_matches_oracle(dev, name, vid):
    """B images in one call, each against its own fp32 oracle run: max-rel < REL, argmax / > threshold agreement > 0.999;
    workspace guards untouched.  Feature-width cases: afterwards a fresh engine samples another, previously verified
    configuration (the smoke test's model at 5 x 7) - an overrun that corrupted a neighbouring allocation has a chance to show."""
    c = S.CASES[name]
    _check_against_oracle(c, _output(name, vid, dev), f'{name}[{vid}]')
    if c['family'] == 'feature_width':
        _check_against_oracle(S.CANARY, _sample(S.CANARY, dev, VARIANTS[(name, vid)][0]), f'canary after {name}[{vid}]')


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
def _launch_counts(eng, x, noise, sn=None):
    """launches per profiler tag of ONE sample() call (prepare() runs before the session is armed)"""
    lib = eng.lib
    eng.prepare()
    torch.cuda.synchronize()
    ms, n = C.c_float(0), C.c_int(0)
    _lib.check(lib.ddp_profile_begin(255), lib)
    try:
        eng.sample(x, noise, sn)
        torch.cuda.synchronize()
    finally:
        rc = lib.ddp_profile_end(C.byref(ms), C.byref(n))
    _lib.check(rc, lib)
    counts = {}
    for tag in range(11):
        _lib.check(lib.ddp_profile_read(tag, C.byref(ms), C.byref(n)), lib)
        counts[tag] = n.value
    return counts


def _expected(path, K, L):
    """Launch counts per tag a path implies, from the launch sites (csrc/ddp_api.hip sample_* / encoder_forward, the prof_begin
    calls of csrc/ddp_gemm_bf16.hip and csrc/ddp_layer_tail.hip).  Tags: 1 x-projection GEMM (256 outputs, TAG_XPROJ), 2 step
    prologue / first head from NCHW (k_layer MODE 2 / 7) and the concat-conv GEMM to SB, 3 layer-0 projection kernel (k_layer
    MODE 3), 7 a plain layer kernel, 8 head GEMMs / seg tails - and EVERY launch_b3_linear of <= 160 outputs or of 256 outputs
    with a tag other than 1 / 3 (launch_b3_linear's dispatch), 10 last layer + tail (k_layer MODE 6 / 8 / 9)."""
    return {
        # xproj hoist; u_0 = W_m . noise is a 256-output GEMM tagged TAG_FEAT, which launch_b3_linear records under 8; layer 0's
        # projections (MODE 3) every step: the BEV head follows a grid resampling
        'bev_chain': {1: 1, 2: 0, 3: K, 7: K * (L - 1), 8: 1, 10: K},
        # the concat-conv GEMM of every step carries TAG_XPROJ; conv_seg is a head GEMM
        'bev_separate': {1: 1 + K, 2: 0, 3: K, 7: K * L, 8: K, 10: 0},
        'seg_head7': {1: 0, 2: 1, 3: 0, 7: K * (L - 1), 8: 0, 10: K},
        'seg_prologue': {1: 1, 2: 1, 3: 0, 7: K * (L - 1), 8: 0, 10: K},
        # once per sample: xproj, rvpad (MODE 3 on xproj), rs0 (96 outputs: recorded under 8); layer 0 is MODE 10 under tag 7
        'depth_chain': {1: 1, 2: 0, 3: 1, 7: K * (L - 1), 8: 1, 10: K},
        'depth_lt': {1: 1, 2: 0, 3: K, 7: K * (L - 1), 8: 0, 10: K},
        'depth_bins': {1: 1, 2: 0, 3: K, 7: K * L, 8: K, 10: 0},
        # DDP_FLAG_UNFUSED_TAIL
        'seg_unfused_tail_head7': {1: 0, 2: 1, 3: 0, 7: K * L, 8: K, 10: 0},
        'seg_unfused_tail_prologue': {1: 1, 2: 1, 3: 0, 7: K * L, 8: K, 10: 0},
        'depth_unfused_tail': {1: 1, 2: 0, 3: K, 7: K * L, 8: K, 10: 0},
    }[path]


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
    got = _launch_counts(eng, x.to(dev), noise.to(dev), sn.to(dev) if sn is not None else None)
    _assert_guards(eng, name)
    want = _expected(c['path'], c['K'], c['L'])
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
    got = _launch_counts(eng, x.to(dev), noise.to(dev))
    want = _expected(path, c['K'], c['L'])
    assert {t: got[t] for t in want} == want, (path, got)


def test_f32_engine_runs_none_of_the_fused_kernels(dev):
    c = S.CASES['bev_kc8_r1']
    _, (x, noise, _) = _state(c)
    got = _launch_counts(_engine(c, dev, 'f32'), x.to(dev), noise.to(dev))
    assert got[10] == 0 and got[2] == 0 and got[8] == c['K'], got        # (its tile GEMMs carry tags 1, 3 .. 8; no k_layer launch exists)
