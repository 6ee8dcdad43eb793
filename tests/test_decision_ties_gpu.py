"""First maximum wins, and ``>`` is strict at the threshold, in every decision kernel - on exact ties.  Needs an MI355X:
``pytest -m gpu``.

The cases of tests/decision_tie_cases.py build ties that are exact in any arithmetic (tests/test_decision_ties_host.py shows on the
CPU that the references see them as such), so every decision assertion here is exact and excuses nothing:

  seg sampler   conv_seg rows of a tie set S zeroed, bias = level: every route that runs the case (the engine variants of
                tests/test_hip_parity.py, ddpm with and without DDP_FLAG_DDPM_CHAIN, the 96-channel step-prologue path, the FCN loop)
                must record min(S) at every token of every step (x0_trace, step record), a step-disagreement map of exactly 0,
                bit-identical result planes over S with argmax min(S), and a result within REL of the fp32 oracle, image by image
                (a padded class column inside the softmax sum shows there); workspace guards untouched.  Reached: the fused seg
                tail (per-lane scan, partner-lane merge, cls < K mask), k_seg_update (f32 engine, unfused tail, ddpm), the tail
                of the FCN loop, the seg branch of k_step_disagreement
  epilogues     duplicated score planes through seg_postprocess (generic and x4 kernels), seg_aug_postprocess (pairs across the
                class ranges of its four waves), seg_slide_postprocess (class map, probabilities, averaged scores) and
                ddp_seg_x0_project: wherever the reference's winner is a member of a pair the GPU class is the LOWER member, and no
                upper member is returned anywhere; elsewhere the MARGIN rule of tests/next_rows_cases.py, its margin taken with
                the duplicates left out; returned probabilities / scores of a pair bit-identical and within REL of the reference
  bev           conv_seg weights zero, biases -8 / 0 / +8 on the u chain (1, 6, 8 classes), the separate kernels (9, 32) and the
                3x3 conv_seg: record bits, ``out > threshold`` and the disagreement map at threshold 0.5 (a probability of exactly
                0.5 is not above it) and at nextafter(0.5, 0) (it is); a 0-bias class comes out as exactly 0.5

One ``TIE <family> <case> <route> ...`` line per test is the record of a run."""
import ctypes as C

import numpy as np
import pytest
import torch

import config_space_cases as S
import decision_tie_cases as T
from ddp_amd import _lib
from golden_util import max_rel
from support import REL, assert_guards, dev, guard, ref_disagreement  # noqa: F401

pytestmark = pytest.mark.gpu


def test_bar_is_the_suite_bar():
    assert T.REL == REL == 2e-4


# ---- 1. the seg sampler -----------------------------------------------------------------------------------------------------------
def _seg_engine(c, route, dev):
    from ddp_amd.engine import DDPEngine, FcnSamplerEngine
    sd = T.seg_state(c)
    if route != 'fcn':
        return guard(DDPEngine(sd, 'seg', device=dev, record_x0=True, record_steps=True, **T.engine_flags(route), **S.engine_kwargs(c)))
    head = T.N.fcn_head(dict(c, classes=c['Kc']), {k[len('decode_head.'):]: v for k, v in sd.items() if k.startswith('decode_head.')}, dev)
    eng = FcnSamplerEngine(sd, head, h=c['h'], w=c['w'], batch=c['B'], randsteps=c['r'], timesteps=c['K'], num_classes=c['Kc'],
                           bit_scale=c['bit_scale'], time_difference=c['td'], sampler=c['sampler'], accumulation=c['accumulation'], device=dev,
                           record_steps=True)
    assert eng._ws_bytes % 4 == 0
    return guard(eng, floats=eng._ws_bytes // 4)         # exactly the queried size (the engine's own allocation has 64 floats of slack)


@pytest.mark.parametrize('name,route', T.seg_pairs())
def test_seg_sampler_takes_the_first_maximum(dev, name, route):
    c = T.route_case(T.SEG[name], route)
    lo, tie = min(c['tie']), list(c['tie'])
    x, noise, sn = T.seg_inputs(c)
    eng = _seg_engine(c, route, dev)
    out = eng.sample(x.to(dev), noise.to(dev), sn.to(dev) if sn is not None else None)
    torch.cuda.synchronize()
    assert_guards(eng, f'{name} {route}')
    out = out.cpu()
    ref = T.seg_oracle(c)['out']
    assert out.shape == ref.shape and torch.isfinite(out).all(), f'{name} {route}: shape or non-finite output'
    rec, dmap = eng.step_record().cpu(), eng.step_disagreement().cpu()
    trace = eng.x0_trace().cpu() if route != 'fcn' else None
    errs = [max_rel(out[b:b + 1], ref[b:b + 1]) for b in range(c['B'])]
    wrong = dict(record=int((rec != lo).sum()), trace=int((trace != lo).sum()) if trace is not None else 0, map=int((dmap != 0).sum()),
                 argmax=int((out.argmax(1) != lo).sum()), planes=sum(int((out[:, k] != out[:, lo]).sum()) for k in tie[1:]))
    tokens = rec.numel()
    print(f'TIE seg {name} {route} K {c["Kc"]} S {tie if len(tie) < 8 else "all"} level {c["level"]:g}: {tokens} decisions checked, 0 excused, '
          f'wrong {wrong}, worst err / REL {max(errs) / REL:.3f}')
    assert tuple(rec.shape) == (c['K'], c['B'], c['r'], c['h'], c['w']) and tuple(dmap.shape) == (c['B'], c['h'], c['w'])
    assert trace is None or tuple(trace.shape) == (c['K'], c['B'] * c['r'], c['h'], c['w'])
    assert not any(wrong.values()), f'{name} {route}: first maximum {lo} expected everywhere; wrong entries {wrong}'
    assert max(errs) < REL, f'{name} {route}: max-rel per image {errs}'


# ---- 2. the epilogues -------------------------------------------------------------------------------------------------------------
def _check_class_map(c, got, what):
    """exact on the pixels a pair wins in the reference, the MARGIN rule with the duplicates left out elsewhere -> (checked, excused)"""
    ref = T.epi_reference(c)
    seg = ref['seg']
    got = got.cpu().long()
    assert got.shape == seg.shape, (got.shape, seg.shape)
    masks, none = T.pair_masks(c, seg)
    for (i, j), m in zip(c['pairs'], masks):
        bad = got[m] != i
        assert not bool(bad.any()), (f'{what}: pair {(i, j)} wins {int(m.sum())} pixels of the reference; on {int(bad.sum())} of them the class is not '
                                     f'{i} (classes seen {sorted(set(got[m][bad].tolist()))})')
    for j in T.upper_planes(c):
        assert not bool((got == j).any()), f'{what}: the upper plane {j} of a pair was returned'
    diff = (got != seg) & none
    if c['kind'] == 'x0':
        assert not bool(diff.any()), f'{what}: {int(diff.sum())} pixels differ from torch.argmax of the same scores'
        return got.numel(), 0
    margin = T.margin_without_duplicates(c, ref['p'])
    share, above = float(diff.float().mean()), int((diff & (margin > T.MARGIN)).sum())
    assert above == 0 and share < T.TIE_SHARE, f'{what}: {share:.2e} of the class map differs, {above} pixels above the margin'
    return got.numel(), int(diff.sum())


def _check_planes(c, got, want, what):
    """returned probabilities / scores: the planes of every pair bit-identical, everything within REL of the reference -> err"""
    got = got.cpu()
    assert got.shape == want.shape and torch.isfinite(got).all(), what
    for i, j in c['pairs']:
        assert torch.equal(got[:, i], got[:, j]), f'{what}: planes {i} and {j} differ in {int((got[:, i] != got[:, j]).sum())} places'
    err = max_rel(got, want)
    assert err < REL, f'{what}: max-rel {err:.3e}'
    return err


def _line(c, route, checked, excused, err=None):
    print(f'TIE epilogue {c["name"]} {route} K {c["K"]} pairs {c["pairs"]}: {checked} pixels checked, {excused} excused' +
          (f', worst err / REL {err / REL:.4f}' if err is not None else ''))


@pytest.mark.parametrize('name', T.epi_names('post'))
def test_seg_postprocess_takes_the_first_maximum(name):
    from ddp_amd.engine import seg_postprocess
    c = T.EPI[name]
    x4 = c['crop'] is None and c['out'] is None and not c['align'] and tuple(c['img']) == (4 * c['h'], 4 * c['w'])
    assert x4 == ('_x4_' in name)          # launch_seg_postprocess (csrc/ddp_kernels.hip): the condition of k_seg_postprocess_x4
    got = seg_postprocess(T.epi_scores(c).cuda(), c['img'], c['crop'], c['out'], c['align'], c['flip'])
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8
    _line(c, 'k_seg_postprocess_x4' if x4 else 'k_seg_postprocess', *_check_class_map(c, got, name))


@pytest.mark.parametrize('name', T.epi_names('aug'))
def test_seg_aug_postprocess_takes_the_first_maximum(name):
    from ddp_amd.engine import seg_aug_postprocess
    c = T.EPI[name]
    scores = [t.cuda() for t in T.epi_scores(c)]
    seg, prob = seg_aug_postprocess(scores, T.aug_metas(c), c['out'], c['align'], return_prob=True)
    alone = seg_aug_postprocess(scores, T.aug_metas(c), c['out'], c['align'])
    torch.cuda.synchronize()
    checked, excused = _check_class_map(c, seg, f'{name} (with probabilities)')
    _check_class_map(c, alone, f'{name} (class map alone)')
    err = _check_planes(c, prob, T.epi_reference(c)['p'], name)
    _line(c, 'k_seg_aug_postprocess', 2 * checked, 2 * excused, err)


@pytest.mark.parametrize('name', T.epi_names('slide'))
def test_seg_slide_postprocess_takes_the_first_maximum(name):
    from ddp_amd.engine import seg_slide_postprocess
    c = T.EPI[name]
    ys, xs, crop = T.N.slide_grid(c)
    args = (torch.stack(T.epi_scores(c)).cuda(), ys, xs, crop, c['img'], c['keep'], c['out'], c['align'])
    seg = seg_slide_postprocess(*args, flip=c['flip'], want='seg')
    prob = seg_slide_postprocess(*args, flip=c['flip'], want='prob')
    raw = seg_slide_postprocess(*args, flip=None, want='scores')
    torch.cuda.synchronize()
    ref = T.epi_reference(c)
    checked, excused = _check_class_map(c, seg, name)
    err = max(_check_planes(c, prob, ref['p'], f'{name} probabilities'), _check_planes(c, raw, ref['raw'], f'{name} averaged scores'))
    _line(c, 'k_seg_slide_postprocess', checked, excused, err)


@pytest.mark.parametrize('name', T.epi_names('x0'))
def test_seg_x0_project_takes_the_first_maximum(dev, name):
    """ddp_seg_x0_project returns the x0 vector of the class it chose: the class is read back as the row of the x0 table the
    vector equals (to REL x bit_scale: the rows are 256 seeded normals apart); no arithmetic precedes the comparison of the
    scores, so the class is torch.argmax of the same scores at EVERY pixel"""
    c = T.EPI[name]
    lib = _lib.load()
    bit_scale = 0.01
    sc, emb = T.epi_scores(c), T.x0_embedding(c)
    B, K, n_pix = c['B'], c['K'], c['h'] * c['w']
    x0 = torch.full((B, 256, n_pix), float('nan'), device=dev)
    dsc, demb = sc.to(dev).contiguous(), emb.to(dev).contiguous()
    _lib.check(lib.ddp_seg_x0_project(dsc.data_ptr(), B, K, n_pix, demb.data_ptr(), C.c_float(bit_scale), x0.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream), lib)
    torch.cuda.synchronize()
    table = T.x0_table(emb, bit_scale)                                   # (K, 256)
    vec = x0.cpu().permute(0, 2, 1)                                      # (B, n, 256)
    assert torch.isfinite(vec).all()
    dist = (vec[:, :, None, :] - table[None, None]).abs().amax(-1)       # (B, n, K)
    near, cls = dist.min(-1)
    assert float(near.max()) <= REL * bit_scale, f'{name}: an x0 vector is no row of the table ({float(near.max()):.3e})'
    assert float(dist.topk(2, dim=-1, largest=False).values[..., 1].min()) > 100 * REL * bit_scale or K < 2
    _line(c, 'k_seg_x0_nchw', *_check_class_map(c, cls.reshape(B, c['h'], c['w']), name), float(near.max()) / bit_scale)


# ---- 3. bev: equality at the threshold --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,vid', T.bev_pairs())
def test_bev_threshold_is_strict(dev, name, vid):
    from ddp_amd.engine import DDPEngine
    c = T.BEV[name]
    kw = dict(T.bev_variants(c))[vid]
    Kc, thr = c['Kc'], c['threshold']
    x, noise, _ = S.inputs(c)
    eng = guard(DDPEngine(T.bev_state(c), 'bev', device=dev, record_steps=True, **kw, **T.bev_engine_kwargs(c)))
    out = eng.sample(x.to(dev), noise.to(dev))
    torch.cuda.synchronize()
    assert_guards(eng, f'{name} {vid}')
    out, rec, dmap = out.cpu(), eng.step_record().cpu(), eng.step_disagreement().cpu()
    o = T.bev_oracle(c)
    assert out.shape == o['out'].shape and torch.isfinite(out).all()
    want = T.bev_expected_bits(c)
    words = rec.long() & 0xFFFFFFFF                                       # (K, B, r, H, W); the C side's uint32
    bits = ((words.unsqueeze(3) >> torch.arange(Kc).view(1, 1, 1, Kc, 1, 1)) & 1).bool()
    assert bits.shape == o['pred'].shape
    zero = T.bev_biases(c) == 0
    above = torch.from_numpy(out.numpy() > np.float32(thr))
    wrong = dict(record=int((bits != want.view(1, 1, 1, Kc, 1, 1)).sum()), record_vs_oracle=int((bits != o['pred']).sum()),
                 high_bits=int(((words >> Kc) != 0).sum()), out=int((above != want.view(1, Kc, 1, 1)).sum()),
                 half=int((out[:, zero] != 0.5).sum()), map=int((dmap != 0).sum()),
                 map_vs_definition=int((dmap.numpy() != ref_disagreement('bev', rec, out, thr)).sum()))
    err = max(max_rel(out[b:b + 1], o['out'][b:b + 1]) for b in range(c['B']))
    print(f'TIE bev {name} {vid} K {Kc} route {c["head_route"]} biases {[int(v) for v in T.bev_biases(c)[:8]]}{"..." if Kc > 8 else ""} threshold '
          f'{thr!r}: {bits.numel() + above.numel()} decisions checked, 0 excused, wrong {wrong}, worst err / REL {err / REL:.4f}')
    assert not any(wrong.values()), f'{name} {vid}: {wrong}'
    assert err < REL
