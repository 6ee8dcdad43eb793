"""DDP_FLAG_DDPM_CHAIN on an MI355X (``pytest -m gpu``): ddpm_sample on the fused step boundary against the CPU oracle at the suite's
bar, against the flag-clear sampler under teacher forcing, and the route, seeded-noise, graph and step-record properties the header
states.  Cases: tests/ddpm_chain_cases.py (tests/test_ddpm_chain_host.py shows on the CPU that the oracle is well conditioned on
each).  Engines sample through guarded, NaN-filled, exactly sized workspaces as in tests/test_config_space_gpu.py."""
import numpy as np
import pytest
import torch

import config_space_cases as S
import ddpm_chain_cases as D
import seeded_noise_util as U
import support
from ddp_amd import _lib
from golden_util import load_case, max_rel
from support import REL, assert_guards, dev, fixture_engine, guard, launch_counts, ref_disagreement, seg_model  # noqa: F401

pytestmark = pytest.mark.gpu

VIDS = D.VIDS
_OUT = {}
_state = support.state_cache(S.state_dict, S.inputs)


def _engine(c, dev, chain=True, gemm='bf16x3', sampler=None, **flags):
    kw = D.engine_kwargs(c)
    if sampler is not None:
        kw['sampler'] = sampler
    eng = support.engine(_state(c)[0], 'seg', kw, dev, gemm, ddpm_chain=chain if kw['sampler'] == 'ddpm' else False, **flags)
    assert bool(eng.cfg.flags & _lib.FLAG_DDPM_CHAIN) == bool(chain and kw['sampler'] == 'ddpm')
    return eng


def _dev_inputs(c, dev):
    _, (x, noise, sn) = _state(c)
    return x.to(dev), noise.to(dev), sn.to(dev)


def _sample(c, dev, chain=True, gemm='bf16x3', **flags):
    eng = _engine(c, dev, chain, gemm, **flags)
    out = eng.sample(*_dev_inputs(c, dev))
    torch.cuda.synchronize()
    assert_guards(eng, c['name'])
    return out.cpu()


def _output(name, vid, dev):
    if (name, vid) not in _OUT:
        _OUT[(name, vid)] = _sample(D.ALL[name], dev, True, **VIDS[vid])
    return _OUT[(name, vid)]


# ---- 1. against the oracle / the reference-made fixture -------------------------------------------------------------------------
def test_bar_is_the_suite_bar():
    assert D.REL == REL == 2e-4


@pytest.mark.parametrize('vid', sorted(VIDS))
@pytest.mark.parametrize('name', sorted(D.ALL))
def test_case_matches_oracle(dev, name, vid):
    D.check_against_oracle(D.ALL[name], _output(name, vid, dev), f'{name}[{vid}]')


@pytest.mark.parametrize('name', sorted(D.ALL))
def test_fused_and_unfused_tail_same_bits(dev, name):
    """k_layer MODE 6 against MODE 0 + MODE 4 / 1 behind the same pre-pass: identical arithmetic, as on the ddim chain"""
    assert torch.equal(_output(name, 'chain', dev), _output(name, 'chain-unfused-tail', dev))


@pytest.mark.parametrize('vid', sorted(VIDS))
def test_fixture_through_the_engine(dev, vid):
    cfg, sd, x, noise, step_noise, g = load_case('seg_ddpm')
    eng = guard(fixture_engine(cfg, sd, dev, ddpm_chain=True, **VIDS[vid]))
    assert eng.cfg.flags & _lib.FLAG_DDPM_CHAIN
    out = eng.sample(x.to(dev), noise.unsqueeze(0).contiguous().to(dev), step_noise.unsqueeze(1).contiguous().to(dev)).cpu()
    assert_guards(eng, 'seg_ddpm')
    err = max_rel(out, g['out'])
    print(f'DDPM-CHAIN fixture seg_ddpm[{vid}]: max-rel {err:.3e} (bar {REL:.0e})')
    assert err < REL


def test_fixture_through_the_plugin(dev):
    cfg, sd, x, noise, step_noise, g = load_case('seg_ddpm')
    model = seg_model(cfg)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    args = dict(noise=noise.unsqueeze(0).to(dev), step_noise=step_noise.unsqueeze(1).to(dev))
    clear = model.ddpm_sample(x.to(dev), None, **args).cpu()
    e0 = next(reversed(model._engine_cache.values()))
    model.ddpm_chain = True
    out = model.ddpm_sample(x.to(dev), None, **args).cpu()
    e1 = next(reversed(model._engine_cache.values()))
    assert e1 is not e0 and (e1.cfg.flags & _lib.FLAG_DDPM_CHAIN) and not (e0.cfg.flags & _lib.FLAG_DDPM_CHAIN)
    assert max_rel(out, g['out']) < REL and max_rel(clear, g['out']) < REL
    # the ddim engine of the same model is not keyed on the attribute's effect
    model.ddim_sample(x.to(dev), None, noise=args['noise'])
    assert not next(reversed(model._engine_cache.values())).cfg.flags & _lib.FLAG_DDPM_CHAIN
    model.ddpm_chain = False
    assert torch.equal(model.ddpm_sample(x.to(dev), None, **args).cpu(), clear)


def test_engine_refuses_the_flag_elsewhere(dev, monkeypatch):
    from ddp_amd.engine import DDPEngine
    c = D.CASES['dc_L1']
    sd = _state(c)[0]
    with pytest.raises(ValueError, match='ddpm_chain'):
        DDPEngine(sd, 'seg', device=dev, ddpm_chain=True, **dict(D.engine_kwargs(c), sampler='ddim'))
    d = S.CASES['depth_K1']
    with pytest.raises(ValueError, match='ddpm_chain'):
        DDPEngine(S.state_dict(d), 'depth', device=dev, ddpm_chain=True, **S.engine_kwargs(d))
    # None reads DDP_DDPM_CHAIN (default off); other samplers ignore the variable
    assert not DDPEngine(sd, 'seg', device=dev, **D.engine_kwargs(c)).cfg.flags & _lib.FLAG_DDPM_CHAIN
    monkeypatch.setenv('DDP_DDPM_CHAIN', '1')
    assert DDPEngine(sd, 'seg', device=dev, **D.engine_kwargs(c)).cfg.flags & _lib.FLAG_DDPM_CHAIN
    assert not DDPEngine(sd, 'seg', device=dev, **dict(D.engine_kwargs(c), sampler='ddim')).cfg.flags & _lib.FLAG_DDPM_CHAIN
    assert not DDPEngine(sd, 'seg', device=dev, ddpm_chain=False, **D.engine_kwargs(c)).cfg.flags & _lib.FLAG_DDPM_CHAIN


@pytest.mark.parametrize('flags', [dict(gemm='f32'), dict(fused_layer=False), dict(fused_prologue=False)], ids=['f32', 'unfused-layer', 'unfused-prologue'])
def test_flag_has_no_effect_off_the_fused_prologue_path(dev, flags):
    c = D.ALL['seg_ddpm_acc']
    assert torch.equal(_sample(c, dev, True, **flags), _sample(c, dev, False, **flags))


# ---- 2. against the flag-clear sampler, teacher forced --------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(D.ALL))
def test_chain_agrees_with_the_flag_clear_sampler_under_teacher_forcing(dev, name):
    """both routes fed the decisions the flag-clear run recorded: no discontinuity is left and the two differ by the regrouping's
    rounding only - max-rel <= 5e-5 (VERDICT.md's figure for this pairing)"""
    c = D.ALL[name]
    x, noise, sn = _dev_inputs(c, dev)
    rec = _engine(c, dev, False, record_x0=True)
    free = rec.sample(x, noise, sn).cpu()
    trace = rec.x0_trace()
    outs = []
    for chain in (False, True):
        eng = _engine(c, dev, chain, force_x0=True)
        eng.set_x0_decisions(trace)
        outs.append(eng.sample(x, noise, sn).cpu())
        torch.cuda.synchronize()
        assert_guards(eng, name)
        if not chain:
            assert torch.equal(eng.x0_trace(), trace) and torch.equal(outs[0], free)     # forcing its own decisions changes nothing
    err = max_rel(outs[1], outs[0])
    print(f'DDPM-CHAIN pair {name}: chain vs flag clear under force_x0 max-rel {err:.3e} (bar {D.CHAIN_VS_CLEAR:.0e})')
    assert err <= D.CHAIN_VS_CLEAR


# ---- 3. route witness -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vid', sorted(VIDS))
@pytest.mark.parametrize('name', sorted(D.ALL))
def test_route_is_the_ddim_chain_plus_the_prepasses(dev, name, vid):
    c = D.ALL[name]
    x, noise, sn = _dev_inputs(c, dev)
    got = launch_counts(_engine(c, dev, True, **VIDS[vid]), x, noise, sn)
    ddim = launch_counts(_engine(c, dev, sampler='ddim', **VIDS[vid]), x, noise)
    print(f'DDPM-CHAIN witness {name}[{vid}]: {got}')
    assert {t: got[t] for t in range(1, 11)} == {t: ddim[t] for t in range(1, 11)}, (got, ddim)
    assert got[0] == D.prepasses(c) == D.NOISE_STEPS[name][0] and ddim[0] == 0
    assert got[10] == (c['K'] if vid == 'chain' else 0) and got[10] + got[8] == c['K']      # the tail kernels do run


@pytest.mark.parametrize('name', ['dc_15tok', 'dc_sr01', 'dc_kc65_r2_nonoise', 'seg_ddpm_acc'])
def test_route_seeded(dev, name):
    """seeded: tag 0 = the start-noise fill + one token-major fill and one pre-pass per noise-adding step that has a next step"""
    c = D.ALL[name]
    x = _dev_inputs(c, dev)[0]
    got = launch_counts(_engine(c, dev, True, seeded_noise=True), x, seed=U.SEED)
    assert got[0] == 1 + 2 * D.prepasses(c), got


@pytest.mark.parametrize('name', ['dc_sr01', 'dc_1x37_r2_cx96', 'seg_ddpm_acc'])
def test_route_flag_clear_is_unchanged(dev, name):
    """flag clear: the separate launches - x-projection GEMM, per step the step prologue, L plain layers and the head GEMM; no tail
    kernel, nothing under tag 0 (the noise transposes and k_seg_update carry no tag)"""
    c = D.ALL[name]
    got = launch_counts(_engine(c, dev, False), *_dev_inputs(c, dev))
    want = {0: 0, 1: 1, 2: c['K'], 3: 0, 7: c['K'] * c['L'], 8: c['K'], 10: 0}
    assert {t: got[t] for t in want} == want, got


# ---- 4. seeded noise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['dc_15tok', 'dc_sr01', 'seg_ddpm_acc'])
def test_seeded_chain_equals_unseeded_chain_fed_the_rebuilt_noise(dev, name):
    """k_noise_fill_tok and the transpose of the caller's tensor feed the pre-pass the same rows: bit for bit.  The step noise is
    rebuilt as in tests/test_seeded_noise_gpu.py (the ddim engine's start-noise fill on stream 1 + s) and checked against the
    restatement of tests/seeded_noise_util.py"""
    c = D.ALL[name]
    x = _dev_inputs(c, dev)[0]
    eng = _engine(c, dev, True, seeded_noise=True)
    out = eng.sample(x, seed=U.SEED, image_base=5, call=2).cpu()
    start = eng.last_noise().clone()
    assert_guards(eng, name)
    ddim = _engine(c, dev, sampler='ddim', seeded_noise=True)
    stack = torch.zeros((c['K'],) + tuple(start.shape), device=dev)
    per = U.per_image(c)
    for s, rec in enumerate(D.records(c)):
        if rec['ddpm_add_noise']:
            ddim.sample(x, seed=U.SEED, image_base=5, call=2, stream_base=1 + s)
            stack[s] = ddim.last_noise()
            ref, rad = U.noise_ref(U.SEED, 5, 1 + s, 2, c['B'], per)
            err = np.abs(stack[s].cpu().numpy().reshape(c['B'], per).astype(np.float64) - ref) / np.maximum(1.0, rad)
            assert err.max() <= U.BOUND_UNIT
    plain = _engine(c, dev, True)
    again = plain.sample(x, start.clone(), stack).cpu()
    assert_guards(plain, name)
    assert torch.equal(again, out)
    if D.prepasses(c):
        assert not torch.equal(plain.sample(x, start.clone(), torch.zeros_like(stack)).cpu(), out)      # the step noise does count
    if name == 'dc_sr01':        # the last step's noise is flagged and must not be read: garbage there changes nothing
        stack[-1] = float('nan')
        assert torch.equal(plain.sample(x, start.clone(), stack).cpu(), out)


# ---- 5. graph ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seeded', [False, True], ids=['unseeded', 'seeded'])
@pytest.mark.parametrize('name', ['dc_15tok', 'seg_ddpm_noacc'])
def test_graph_capture_and_replay_same_bits(dev, name, seeded):
    c = D.ALL[name]
    x, noise, sn = _dev_inputs(c, dev)
    eng = _engine(c, dev, True, seeded_noise=seeded)
    if seeded:
        want = eng.sample(x, seed=U.SEED, image_base=3, call=1).clone()
        g = eng.capture(x, seed=U.SEED, image_base=3, call=1)
        got = g.replay(x).clone()
        other = g.replay(x, seed=U.SEED_B).clone()
        assert torch.equal(other, eng.sample(x, seed=U.SEED_B, image_base=3, call=1))
    else:
        want = eng.sample(x, noise, sn).clone()
        g = eng.capture(x, noise, sn)
        got = g.replay(x, noise, sn).clone()
        other = None
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(g.replay().clone(), other if seeded else want)       # (seeded: replay() alone repeats the LAST key)
    assert_guards(eng, name)


# ---- 6. step record ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('vid', sorted(VIDS))
@pytest.mark.parametrize('name', ['dc_15tok', 'dc_1x37_r2_cx96', 'seg_ddpm_acc'])
def test_step_record_is_the_x0_trace_and_the_map_its_definition(dev, name, vid):
    c = D.ALL[name]
    x, noise, sn = _dev_inputs(c, dev)
    rec = _engine(c, dev, True, record_steps=True, **VIDS[vid])
    out = rec.sample(x, noise, sn).cpu()
    assert_guards(rec, name)
    assert torch.equal(out, _output(name, vid, dev))                       # the flag does not move the output
    record, smap = rec.step_record().cpu(), rec.step_disagreement().cpu()
    assert record.shape == (c['K'], c['B'], c['r'], c['h'], c['w']) and record.dtype == torch.uint8
    tr = _engine(c, dev, True, record_x0=True, **VIDS[vid])
    assert torch.equal(tr.sample(x, noise, sn).cpu(), out)
    assert torch.equal(tr.x0_trace().cpu().reshape(record.shape), record)
    want = ref_disagreement('seg', record, out)
    assert np.array_equal(smap.numpy(), want)
    # the last step's record is the argmax of the last step's scores: without accumulation, of the output's replicas' mean only at r = 1
    if not c['accumulation'] and c['r'] == 1:
        assert torch.equal(record[-1, :, 0].long(), out.argmax(1))
