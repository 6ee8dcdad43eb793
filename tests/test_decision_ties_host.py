"""The conditions that keep tests/test_decision_ties_gpu.py honest, on the CPU (no GPU needed).  Conditions, not measurements:

  sampler cases   the fp32 and the fp64 oracle give the scores of the tie set EXACTLY the level at every step, every other class at
                  least 16 lower (far beyond any rounding of a score that is not tied); the oracle's own argmax is min(S) at every
                  step; the fp32 oracle's result is within COND = REL / 20 of its fp64 evaluation - under ddim and, for the cases
                  the ddpm routes run, under ddpm
  epilogue cases  the duplicated planes are bit-identical in the tensor the reference takes its argmax of; torch.argmax never
                  returns the upper plane; every pair wins >= 10 % of the pixels; no pixel a pair wins has a reference near-tie
                  with a third class (so the GPU assertion there needs no allowance); elsewhere the share of pixels the MARGIN rule
                  of tests/next_rows_cases.py excuses is below its TIE_SHARE
  bev cases       torch.sigmoid(0) is exactly 0.5; the oracle's thresholded maps are the expected bits at every step; its result for
                  a 0-bias class is exactly 0.5; the restatement used for the per-step maps gives the oracle's bits
  all             every case builds deterministically; the route list is tests/test_hip_parity.py VARIANTS plus the four named
                  extras, every route has cases and every case a route"""
import numpy as np
import pytest
import torch

import decision_tie_cases as T
from golden_util import max_rel
from support import VARIANTS as PARITY_VARIANTS


def test_constants_are_the_suites():
    import config_space_cases as S
    import next_rows_cases as N
    from support import REL
    assert T.REL == REL == S.REL == 2e-4 and T.COND == S.COND == REL / 20
    assert T.MARGIN == N.MARGIN and T.TIE_SHARE == N.TIE_SHARE


def test_route_list_is_the_parity_variants_plus_the_named_extras():
    assert set(T.ROUTES) == set(PARITY_VARIANTS) | {'ddpm', 'ddpm-chain', 'cx96', 'fcn'} and len(T.ROUTES) == len(PARITY_VARIANTS) + 4
    pairs = T.seg_pairs()
    for r in T.ROUTES:
        assert any(rr == r for _, rr in pairs), f'route {r} runs no case'
    for n in T.SEG:
        assert any(nn == n for nn, _ in pairs), f'case {n} runs on no route'
    for v in PARITY_VARIANTS:
        assert T.engine_flags(v) == PARITY_VARIANTS[v]
    assert T.engine_flags('ddpm') == dict(gemm='bf16x3', ddpm_chain=False) and T.engine_flags('ddpm-chain') == dict(gemm='bf16x3', ddpm_chain=True)
    assert sum(c['Cx'] == 96 for c in T.SEG.values()) == 1


def test_case_lists_cover_what_they_name():
    kcs = {c['Kc'] for c in T.SEG.values() if c['head'] == 'deformable'}
    assert kcs == {2, 19, 64, 65, 150, 193, 256}
    assert {c['level'] for c in T.SEG.values()} == {0.0, 3.0}
    ties = {c['tie'] for c in T.SEG.values()}
    for want in ((1, 2), (3, 4), (7, 8), (31, 32), (63, 64), (127, 128), (191, 192), (5, 69), (5, 197), (36, 100, 229)):
        assert want in ties, want
    for kc in kcs - {2}:
        assert any(c['Kc'] == kc and c['tie'] == (kc - 2, kc - 1) for c in T.SEG.values()), kc
        assert any(c['Kc'] == kc and c['tie'] == (4, kc - 1) for c in T.SEG.values()), kc
    assert any(len(c['tie']) == c['Kc'] == 256 for c in T.SEG.values())
    assert any(c['r'] == 2 for c in T.SEG.values()) and any(not c['accumulation'] for c in T.SEG.values())
    assert all((c['B'], c['h'], c['w'], c['L'], c['K'], c['td']) == (2, 5, 7, 2, 3, 1) for c in T.SEG.values())
    assert {c['K'] for c in T.EPI.values()} == {2, 19, 150, 256} and {c['kind'] for c in T.EPI.values()} == {'post', 'aug', 'slide', 'x0'}
    assert {(c['Kc'], c['head_route']) for c in T.BEV.values()} == {(1, 'bev_chain'), (6, 'bev_chain'), (8, 'bev_chain'), (9, 'bev_separate'),
                                                                    (32, 'bev_separate'), (6, 'seg3'), (9, 'seg3')}
    assert T.THRESHOLDS['below_half'] == float(np.nextafter(np.float32(0.5), np.float32(0))) < 0.5


def test_bev_bias_patterns_reach_every_bit_position():
    for kc in (1, 6, 8, 9, 32):
        cases = [c for c in T.BEV.values() if c['Kc'] == kc and c['seg_kernel'] == 1 and c['thr_name'] == 'half' and c['r'] == 1]
        assert len(cases) == 3
        assert {float(T.bev_biases(c)[0]) for c in cases} == set(T.BIAS_VALUES) == {float(T.bev_biases(c)[kc - 1]) for c in cases}
        if kc >= 6:
            for c in cases:
                b = T.bev_biases(c)[:8]
                halves = [{float(v) for k, v in enumerate(b) if (k >> 2) & 1 == h} for h in (0, 1)]
                assert halves[0] == set(T.BIAS_VALUES) and (kc < 8 or halves[1] == set(T.BIAS_VALUES)), (kc, halves)


def _samplers(c):
    return ['ddim'] + (['ddpm'] if T.accepts(c, 'ddpm') else [])


@pytest.mark.parametrize('name', list(T.SEG))
def test_sampler_case_conditions(name):
    c0 = T.SEG[name]
    tie, lo = list(c0['tie']), min(c0['tie'])
    rest = [k for k in range(c0['Kc']) if k not in set(tie)]
    for sampler in _samplers(c0):
        c = dict(c0, sampler=sampler)
        o32, o64 = T.seg_oracle(c), T.seg_oracle(c, torch.float64)
        for o in (o32, o64):
            assert len(o['logits']) == c['B']
            for steps in o['logits']:
                assert len(steps) == c['K']
                for lg in steps:
                    assert tuple(lg.shape) == (c['r'], c['Kc'], c['h'], c['w'])
                    assert bool((lg[:, tie] == c['level']).all()), f'{name} {sampler}: a tied score is not exactly the level'
                    if rest:
                        assert float(lg[:, rest].max()) <= c['level'] - T.MIN_GAP, f'{name} {sampler}: {float(lg[:, rest].max())}'
                    assert bool((lg.argmax(1) == lo).all())
            assert bool((o['out'].argmax(1) == lo).all())
            for k in tie[1:]:
                assert torch.equal(o['out'][:, k], o['out'][:, lo])
        cond = max_rel(o32['out'], o64['out'].float())
        assert cond <= T.COND, f'{name} {sampler}: fp32 oracle {cond:.3e} from its fp64 evaluation'


@pytest.mark.parametrize('name', T.epi_names())
def test_epilogue_case_conditions(name):
    c = T.EPI[name]
    ref = T.epi_reference(c)
    p, seg = ref['p'], ref['seg']
    for key in ('p', 'raw'):
        if key in ref:
            for i, j in c['pairs']:
                assert torch.equal(ref[key][:, i], ref[key][:, j]), f'{name}: planes {i} and {j} of the reference differ'
    assert torch.equal(seg, p.argmax(1))
    if c['kind'] != 'x0':
        # the padded evaluation (decision_tie_cases.epi_reference) is the plain one up to the rounding of torch's scalar tail loop
        plain = T.epi_reference(c, pad=False)
        for key in ('p', 'raw'):
            if key in ref:
                assert float((ref[key] - plain[key]).abs().max()) <= T.MARGIN * max(1.0, float(plain[key].abs().max()))
        if c['K'] % 8 == 0:
            assert torch.equal(ref['p'], plain['p']) and torch.equal(seg, plain['seg'])
    masks, none = T.pair_masks(c, seg)
    for (i, j), m in zip(c['pairs'], masks):
        assert not bool((seg == j).any()), f'{name}: torch.argmax returned the upper plane {j}'
        assert float(m.float().mean()) >= T.MIN_WIN, f'{name}: pair {(i, j)} wins {float(m.float().mean()):.3f} of the pixels'
    if c['kind'] == 'x0':
        return                                   # (no arithmetic in front of the comparison: the GPU test asserts every pixel)
    margin = T.margin_without_duplicates(c, p)
    assert int(((margin <= T.MARGIN) & ~none).sum()) == 0, f'{name}: a near-tie with a third class on a pixel a pair wins'
    assert float(((margin <= T.MARGIN) & none).float().mean()) < T.TIE_SHARE


@pytest.mark.parametrize('name', list(T.BEV))
def test_bev_case_conditions(name):
    c = T.BEV[name]
    assert float(torch.sigmoid(torch.zeros(1))) == 0.5 and float(torch.sigmoid(torch.zeros(1, dtype=torch.float64))) == 0.5
    o = T.bev_oracle(c)
    want = T.bev_expected_bits(c)
    assert want.any() or c['Kc'] == 1
    K, B, r, Kc, H, W = o['pred'].shape
    assert (K, B, r, Kc) == (c['K'], c['B'], c['r'], c['Kc'])
    assert torch.equal(o['pred'], want.view(1, 1, 1, Kc, 1, 1).expand_as(o['pred']))
    assert torch.equal(o['out'] > c['threshold'], want.view(1, Kc, 1, 1).expand_as(o['out']))
    zero = T.bev_biases(c) == 0
    assert bool((o['out'][:, zero] == 0.5).all())
    assert torch.equal(o['out'], o['restated'])


def test_cases_build_deterministically():
    for c in [T.SEG['k193_s63_64_191_192_l0'], T.SEG['k19_s3_4_l0_fcn'], T.SEG['k150_s63_64_l0_cx96']]:
        a, b = T.seg_state(c), T.seg_state(c)
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
        for ta, tb in zip(T.seg_inputs(dict(c, sampler='ddpm')), T.seg_inputs(dict(c, sampler='ddpm'))):
            assert torch.equal(ta, tb)
    for c in T.EPI.values():
        a, b = T.epi_scores(c), T.epi_scores(c)
        a, b = (a, b) if isinstance(a, list) else ([a], [b])
        assert all(torch.equal(p, q) for p, q in zip(a, b))
    for c in list(T.BEV.values())[::7]:
        a, b = T.bev_state(c), T.bev_state(c)
        assert all(torch.equal(a[k], b[k]) for k in a)


def test_sampler_tie_construction_touches_conv_seg_only():
    c = T.SEG['k150_s5_69_l0']
    from ddp_amd.utils import synthetic
    base, sd = synthetic.make_state_dict('seg', 150, 2, 256, seed=c['seed']), T.seg_state(c)
    for k in base:
        if not k.startswith('decode_head.conv_seg.'):
            assert torch.equal(base[k], sd[k]), k
    w, b = sd['decode_head.conv_seg.weight'], sd['decode_head.conv_seg.bias']
    assert float(w[[5, 69]].abs().max()) == 0.0 and b[5] == b[69] == 0.0
    keep = [k for k in range(150) if k not in (5, 69)]
    assert torch.equal(w[keep], base['decode_head.conv_seg.weight'][keep])
    assert torch.equal(b[keep], base['decode_head.conv_seg.bias'][keep] + T.OTHERS)
