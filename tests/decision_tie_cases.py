"""Exact ties in every decision kernel: the cases, the references and the conditions shared by tests/test_decision_ties_gpu.py
(GPU: first maximum wins, strict '>' at the threshold, on every route) and tests/test_decision_ties_host.py (CPU: the conditions
that make those expectations unambiguous).  Imports no GPU.

Every other parity test draws random scores, which never tie, and excuses near-ties; the promise of include/ddp_mi355x.h ("first
maximum wins", ``> threshold``) is kept by a different reduction in every kernel.  Three families build ties that are exact in ANY
arithmetic, so the expectation needs no tolerance:

  SEG    sampler cases.  A seeded ``synthetic`` model whose ``conv_seg`` rows of a tie set S are zero with bias ``level``, every
         other class 64 lower: the scores of S are exactly ``level`` (a sum of exact zeros plus the bias) in fp32, fp64, the bf16x3
         split and the fp32 MFMA alike, at every token, step and replica, whatever the accumulation order.  Expected decision:
         min(S).  ``level`` 0.0 ties S with the padded columns >= K of the tall stages as well (zero weights, zeroed bias table).
         70 tokens (B 2, 5 x 7): three 32-token groups, the last partial; three steps: prob_mode 1 then 2.  A class lives at
         chunk c = k >> 6, tile t = (k >> 5) & 1, g = (k >> 3) & 3, half-wave h = (k >> 2) & 1, e = k & 3 of the fused tail
         (csrc/layer_bf16x3.h); the tie sets put winner and loser on either side of each of those boundaries.
  EPI    the epilogues that take (B, K, h, w) scores.  Random planes; for disjoint pairs (i, j), i < j, plane i is copied into plane
         j and one offset added to both: every arithmetic step of the epilogues is per plane, so the two stay bit-identical through
         both resizes, the window averaging and the softmax, and torch.argmax of the reference never returns j - once the
         reference is evaluated with every plane in a vector position of torch's CPU resize (``epi_reference``: classes padded).
  BEV    conv_seg weights zero, biases from {-8, 0, +8}: the score is the bias.  sigmoid(0) is exactly 0.5, which is not > 0.5;
         at threshold nextafter(0.5, 0) it is.

Routes of a SEG case (``ROUTES``): the engine variants of tests/test_hip_parity.py (all of them: the host test pins the list), the
ddpm sampler with and without DDP_FLAG_DDPM_CHAIN, one 96-channel case on the step-prologue path, the FCN loop.

Seeds: every case takes the next seed of its family, except the epilogue cases noted at ``EPI_RESEED`` (host conditions: no
reference near-tie may sit on a pixel a duplicated pair wins, every pair wins >= 10 % of the pixels)."""
import numpy as np
import torch
import torch.nn.functional as F

import config_space_cases as S
import next_rows_cases as N
from config_space_cases import COND, REL  # noqa: F401  (the suite bar and the conditioning rule, not restated)
from ddp_amd.utils import synthetic
from next_rows_cases import MARGIN, TIE_SHARE  # noqa: F401
from oracle import ddp_oracle as O
from support import VARIANTS as PARITY_VARIANTS

OTHERS = -64.0            # added to the bias of every class outside the tie set
MIN_GAP = 16.0            # every other class sits at least this far under the level (host condition; far beyond any rounding)
MIN_WIN = 0.10            # share of the pixels every duplicated pair must win in the reference
EXTRA_ROUTES = ('ddpm', 'ddpm-chain', 'cx96', 'fcn')
ROUTES = tuple(PARITY_VARIANTS) + EXTRA_ROUTES

# ---- 1. sampler cases -------------------------------------------------------------------------------------------------------------
SEG = {}


def _seg(Kc, tie, level, tag='', **kw):
    tie = tuple(range(Kc)) if tie == 'all' else tuple(sorted(tie))
    assert len(tie) >= 2 and tie[-1] < Kc
    what = 'all' if len(tie) == Kc and Kc > 4 else '_'.join(str(k) for k in tie)
    name = f'k{Kc}_s{what}_l{level:g}{tag}'
    c = dict(name=name, family='tie_seg', task='seg', B=2, r=1, K=3, L=2, Cx=256, td=1, h=5, w=7, Kc=Kc, bit_scale=0.01, accumulation=True,
             sampler='ddim', head='deformable', tie=tie, level=float(level), seed=1300 + len(SEG))
    c.update(kw)
    assert name not in SEG
    SEG[name] = c


# {1,2} same lane, adjacent e; {3,4} h flips (partner-lane merge); {7,8} g; {31,32} t; {63,64} {127,128} {191,192} chunk c;
# {5,69} {5,197} same slot, other chunk; {K-2,K-1}; {4,K-1} lower class in the partner lane's half; {36,100,229}; all classes
_seg(2, 'all', 0.0)
_seg(2, 'all', 3.0)
_seg(19, (1, 2), 0.0)
_seg(19, (3, 4), 3.0)
_seg(19, (7, 8), 0.0)
_seg(19, (17, 18), 3.0)
_seg(19, (4, 18), 0.0)
_seg(19, 'all', 3.0)
_seg(64, (31, 32), 0.0)
_seg(64, (62, 63), 3.0)
_seg(64, (4, 63), 0.0)
_seg(64, (7, 8), 3.0)
_seg(65, (63, 64), 0.0)
_seg(65, (4, 64), 3.0)
_seg(65, (31, 32), 3.0)
_seg(65, (1, 2), 3.0)
_seg(150, (63, 64), 3.0)
_seg(150, (127, 128), 0.0)
_seg(150, (5, 69), 0.0)
_seg(150, (148, 149), 3.0)
_seg(150, (4, 149), 0.0)
_seg(150, (36, 100), 3.0)
_seg(150, (3, 4), 0.0)
_seg(193, (191, 192), 0.0)
_seg(193, (127, 128), 3.0)
_seg(193, (5, 69), 3.0)
_seg(193, (63, 64, 191, 192), 0.0)
_seg(193, (4, 192), 3.0)
_seg(256, (191, 192), 3.0)
_seg(256, (5, 197), 0.0)
_seg(256, (254, 255), 0.0)
_seg(256, (4, 255), 3.0)
_seg(256, (36, 100, 229), 0.0)
_seg(256, 'all', 0.0)
_seg(256, (5, 69), 3.0)
_seg(150, (127, 128), 0.0, tag='_r2', r=2)                        # two replicas: 140 rows, the mean over K r maps
_seg(19, (3, 4), 0.0, tag='_noacc', accumulation=False)          # prob_mode 0 then 3: the result is the last step's scores
_seg(150, (63, 64), 0.0, tag='_cx96', Cx=96)                      # x-projection GEMM + step prologue in front of the chain
for _kc, _tie, _lv in ((19, (3, 4), 0.0), (65, (63, 64), 3.0), (150, (4, 149), 0.0), (256, (36, 100, 229), 3.0), (256, 'all', 0.0)):
    _seg(_kc, _tie, _lv, tag='_fcn', head='fcn', num_convs=2, dilation=1, bn=True)


def accepts(c, route):
    """does ``route`` run the sampler case ``c``?  (the flags act on the bf16x3 engine of the deformable head; DDP_FLAG_SB_HEAD and
    the NCHW step head exist at 256 feature channels and r = 1, tests/test_config_space_gpu.py::variants)"""
    if c['head'] == 'fcn':
        return route == 'fcn'
    if c['Cx'] != 256:
        return route == 'cx96'
    if route in ('fcn', 'cx96'):
        return False
    return c['r'] == 1 or route != 'bf16x3-sb-head'


def route_case(c, route):
    """the case as the route runs it (the ddpm routes: the same model and start noise, the ddpm update, seeded step noise)"""
    return dict(c, sampler='ddpm') if route in ('ddpm', 'ddpm-chain') else c


def engine_flags(route):
    """DDPEngine keyword arguments of a route (not of the FCN loop)"""
    if route in PARITY_VARIANTS:
        return dict(PARITY_VARIANTS[route])
    return dict(gemm='bf16x3', **({'ddpm_chain': route == 'ddpm-chain'} if route in ('ddpm', 'ddpm-chain') else {}))


def seg_pairs():
    return [(n, r) for n, c in SEG.items() for r in ROUTES if accepts(c, r)]


def _tie_head(sd, c, wkey, bkey):
    w, b = sd[wkey].clone(), sd[bkey].clone()
    inside = torch.zeros(c['Kc'], dtype=torch.bool)
    inside[list(c['tie'])] = True
    w[inside] = 0.0
    b[inside] = c['level']
    b[~inside] += OTHERS
    sd[wkey], sd[bkey] = w, b
    return sd


def seg_state(c):
    """the seeded model of the case with its conv_seg tied (fp32, CPU); FCN cases: the segmentor around FCNHeadWithTime"""
    if c['head'] == 'fcn':
        sd = N.loop_state(dict(classes=c['Kc'], Cx=256, seed=c['seed'], num_convs=c['num_convs'], bn=c['bn']))
    else:
        sd = synthetic.make_state_dict('seg', c['Kc'], c['L'], c['Cx'], seed=c['seed'])
    return _tie_head(sd, c, 'decode_head.conv_seg.weight', 'decode_head.conv_seg.bias')


def seg_inputs(c):
    """-> x (B,Cx,h,w), noise (B,r,256,h,w), step noise (K,B,r,256,h,w) or None (config_space_cases.inputs)"""
    return S.inputs(c)


_SEG_ORACLE = {}


def seg_oracle(c, dtype=torch.float32):
    """-> dict(out (B,Kc,h,w), logits [B][K] of (r,Kc,h,w)): the reference sampler of the case, image by image, with the scores of
    every step kept (through the oracle's own ``head`` hook: nothing of its arithmetic changes).  Once per (case, sampler, dtype)."""
    key = (c['name'], c['sampler'], dtype)
    if key in _SEG_ORACLE:
        return _SEG_ORACLE[key]
    sd = {k: v.to(dtype) for k, v in seg_state(c).items()}
    x, noise, sn = seg_inputs(c)
    outs, logits = [], []
    for b in range(c['B']):
        steps = []
        if c['head'] == 'fcn':
            inner = O.fcn_head_for_sampler(sd, c['num_convs'], c['dilation'])
        else:
            def inner(feat, temb):
                return O.head_forward_seg(feat, temb, sd)

        def head(feat, temb):
            steps.append(inner(feat, temb))
            return steps[-1]
        kw = dict(timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'], time_difference=c['td'], accumulation=c['accumulation'], head=head)
        with torch.no_grad():
            if c['sampler'] == 'ddpm':
                outs.append(O.ddpm_sample_seg(x[b:b + 1].to(dtype), noise[b].to(dtype), sn[:, b].to(dtype), sd, **kw))
            else:
                outs.append(O.ddim_sample_seg(x[b:b + 1].to(dtype), noise[b].to(dtype), sd, **kw))
        logits.append(steps)
    _SEG_ORACLE[key] = dict(out=torch.cat(outs, dim=0), logits=logits)
    return _SEG_ORACLE[key]


# ---- 2. epilogues: duplicated score planes ----------------------------------------------------------------------------------------
EPI = {}
MAP = (9, 13)
# seeds that differ from the running number, as case: what is added to it - the first of the scan + 0, + 100, + 200 ... that meets
# the host conditions (tests/test_decision_ties_host.py::test_epilogue_case_conditions); with the running number each of these
# cases has one pixel where two PAIRS are within MARGIN of each other in the reference
EPI_RESEED = {'post_k19_ac0_horizontal': 100, 'post_k150_ac1_noflip': 100, 'post_k150_ac0_horizontal': 200, 'post_k256_ac1_horizontal': 100,
              'post_k19_first_last': 100, 'aug_k150_waves': 100}


def generic_pairs(K):
    if K == 2:
        return [(0, 1)]
    return [(4, 11), (17, 18)] if K == 19 else [(4, 11), (17, 18), (0, K - 1)]


def wave_pairs(K):
    """pairs across the class ranges kq = (K + 3) >> 2 that k_seg_aug_postprocess gives its four waves"""
    kq = (K + 3) >> 2
    return [(0, 1)] if K == 2 else [(kq - 1, kq), (2 * kq - 1, 3 * kq), (0, K - 1)]


def _epi(name, kind, K, pairs, offset=6.0, **kw):
    assert name not in EPI
    flat = [k for p in pairs for k in p]
    assert len(set(flat)) == len(flat) and all(0 <= i < j < K for i, j in pairs), (name, pairs)
    c = dict(name=name, family='tie_epilogue', kind=kind, B=2, K=K, h=MAP[0], w=MAP[1], pairs=list(pairs), offset=offset,
             seed=2000 + len(EPI) + EPI_RESEED.get(name, 0))
    c.update(kw)
    EPI[name] = c


for _k in (2, 19, 150, 256):
    for _fl in (None, 'horizontal', 'vertical'):
        _f = _fl or 'noflip'
        _epi(f'post_x4_k{_k}_{_f}', 'post', _k, generic_pairs(_k), img=(36, 52), crop=None, out=None, align=False, flip=_fl)
        for _ac in (False, True):
            _epi(f'post_k{_k}_ac{int(_ac)}_{_f}', 'post', _k, generic_pairs(_k), img=(36, 52), crop=(33, 50), out=(41, 67), align=_ac, flip=_fl)
_epi('post_k19_first_last', 'post', 19, [(0, 18), (4, 11)], img=(36, 52), crop=(33, 50), out=(41, 67), align=False, flip=None)
_epi('post_x4_k19_first_last', 'post', 19, [(0, 18), (4, 11)], img=(36, 52), crop=None, out=None, align=False, flip=None)
# three augmentations of different scale, one flipped (network input 4 x the map, the second one cropped)
_AUGS = [dict(h=9, w=13, crop_cut=(0, 0), flip=None), dict(h=7, w=10, crop_cut=(2, 1), flip='horizontal'), dict(h=12, w=17, crop_cut=(1, 3), flip=None)]
for _k in (2, 19, 150, 256):
    _epi(f'aug_k{_k}_waves', 'aug', _k, wave_pairs(_k), out=(30, 45), align=False, augs=_AUGS)
    if _k > 2:
        _epi(f'aug_k{_k}_generic', 'aug', _k, generic_pairs(_k), out=(30, 45), align=bool(_k == 19), augs=_AUGS)
# a 2 x 2 window grid with overlap: windows of 20 x 32 at stride 10 x 16 on a 30 x 48 image, window maps of 5 x 8 (the entry
# wants every window's scores 16-byte aligned, and ddp_amd.engine.seg_slide_postprocess takes them as slices of one tensor: B K h w
# has to be a multiple of 4)
for _k in (2, 19, 150, 256):
    for _fl in ((None, 'horizontal') if _k in (19, 256) else (None,)):
        _epi(f'slide_k{_k}_{_fl or "noflip"}', 'slide', _k, generic_pairs(_k), h=5, w=8, img=(30, 48), crop_size=(20, 32), stride=(10, 16),
             keep=(29, 46), out=(33, 47), align=False, flip=_fl)
for _k in (2, 19, 150, 256):
    _epi(f'x0_k{_k}', 'x0', _k, generic_pairs(_k), h=23 if _k == 19 else 9)          # 299 pixels: more than one block


def epi_names(kind=None):
    return [n for n, c in EPI.items() if kind is None or c['kind'] == kind]


def duplicate(scores, c):
    """plane i copied into plane j, the case's offset added to both, for every pair of the case"""
    out = scores.clone()
    for i, j in c['pairs']:
        out[:, i] = scores[:, i] + c['offset']
        out[:, j] = out[:, i]
    return out


def upper_planes(c):
    return [j for _, j in c['pairs']]


def epi_scores(c):
    """'post' / 'x0': (B,K,h,w); 'aug': list of (B,K,h_i,w_i); 'slide': list of four window maps (B,K,h,w)"""
    if c['kind'] == 'aug':
        return [duplicate(synthetic.make_scores(c['B'], c['K'], a['h'], a['w'], c['seed'] * 100 + i), c) for i, a in enumerate(c['augs'])]
    if c['kind'] == 'slide':
        ys, xs, _ = N.slide_grid(c)
        return [duplicate(synthetic.make_scores(c['B'], c['K'], c['h'], c['w'], c['seed'] * 100 + i), c) for i in range(len(ys) * len(xs))]
    return duplicate(synthetic.make_scores(c['B'], c['K'], c['h'], c['w'], c['seed']), c)


def aug_metas(c):
    return [dict(img_size=(4 * a['h'], 4 * a['w']), crop_size=(4 * a['h'] - a['crop_cut'][0], 4 * a['w'] - a['crop_cut'][1]), flip=a['flip'])
            for a in c['augs']]


PAD_TO = 32               # classes of the reference's input, rounded up (see epi_reference)
PAD_SCORE = -1e4          # score of the planes added for that: exp(PAD_SCORE - max) is exactly 0 in fp32 and fp64


def pad_classes(sc):
    """(B, K, h, w) -> (B, K rounded up to PAD_TO, h, w), the added planes at PAD_SCORE"""
    B, K, h, w = sc.shape
    kp = -(-K // PAD_TO) * PAD_TO
    return sc if kp == K else torch.cat([sc, torch.full((B, kp - K, h, w), PAD_SCORE, dtype=sc.dtype)], dim=1)


_EPI_REF = {}


def epi_reference(c, pad=True):
    """-> dict(seg int64 class map, p the tensor its argmax is taken of[, raw: the window-averaged scores]): the composition the
    epilogue tests of tests/test_next_rows_gpu.py use - the oracle and torch ops on the CPU, then torch.argmax.  Once per case.

    ``pad``: the oracle runs on the scores with planes of PAD_SCORE appended up to a multiple of PAD_TO classes, and the result
    is cut back to K.  The appended planes never win and add exactly 0 to every softmax sum, so this is the same composition;
    what it changes is how torch evaluates it.  ``F.interpolate`` on the CPU walks the channels in vectors (of 8 floats here) and
    finishes the K % 8 last ones in a scalar loop that rounds differently (measured on torch 2.10: planes 16 .. 18 of 19 and
    144 .. 149 of 150 come out up to 1 ulp from what the same plane gives in a vector position, at every size of this file;
    K = 2 and 256 have no such tail).  Unpadded, plane K - 1 of a pair (0, K - 1) is therefore not bit-identical to plane 0 in the
    REFERENCE, and its argmax returns either member.  Padded, every real plane sits in a vector position; the host test asserts
    that the duplicated planes of the reference are then bit-identical and that the padded evaluation is within MARGIN of the
    plain one."""
    if (c['name'], pad) in _EPI_REF:
        return _EPI_REF[(c['name'], pad)]
    sc = epi_scores(c)
    K = c['K']
    fit = pad_classes if pad else (lambda t: t)
    with torch.no_grad():
        if c['kind'] == 'post':
            p = N.post_probs(c, fit(sc))
            res = dict(seg=O.seg_postprocess(fit(sc), c['img'], c['crop'], c['out'], c['align'], c['flip']), p=p[:, :K])
        elif c['kind'] == 'aug':
            seg, p = O.seg_aug_test([fit(t) for t in sc], aug_metas(c), c['out'], c['align'])
            res = dict(seg=seg, p=p[:, :K])
        elif c['kind'] == 'slide':
            ys, xs, crop = N.slide_grid(c)
            raw = O.seg_slide_inference([fit(t) for t in sc], ys, xs, crop, c['img'], c['keep'], c['out'], c['align'])
            p = torch.softmax(raw, dim=1)
            if c['flip']:
                p = p.flip(dims=(3,) if c['flip'] == 'horizontal' else (2,))
            res = dict(seg=p.argmax(1), p=p[:, :K], raw=raw[:, :K])
        else:
            res = dict(seg=sc.argmax(1), p=sc)
    _EPI_REF[(c['name'], pad)] = res
    return res


def pair_masks(c, seg):
    """-> (per pair: pixels of ``seg`` where one of its members wins, pixels where no pair wins)"""
    masks = [(seg == i) | (seg == j) for i, j in c['pairs']]
    none = torch.ones_like(masks[0])
    for m in masks:
        none &= ~m
    return masks, none


def margin_without_duplicates(c, p):
    """top-2 margin of (B, K, ...) with the upper plane of every pair left out: an exact tie cannot hide in the near-tie allowance"""
    keep = [k for k in range(p.shape[1]) if k not in set(upper_planes(c))]
    return N.top2_margin(p[:, keep])


def x0_table(emb, bit_scale):
    """(K, 256): the x0 vector of every class (segmentors/ddp.py:235-237)"""
    return (torch.sigmoid(emb) * 2 - 1) * bit_scale


def x0_embedding(c):
    g = torch.Generator().manual_seed(c['seed'] + 7)
    return torch.randn((c['K'], 256), generator=g)


# ---- 3. BEV threshold equality ----------------------------------------------------------------------------------------------------
BEV = {}
BIAS_VALUES = (-8.0, 0.0, 8.0)
THRESHOLDS = {'half': 0.5, 'below_half': float(np.nextafter(np.float32(0.5), np.float32(0.0)))}
_BEV_BASE = dict(S.CASES['bev_kc5_th0.3'], L=2, K=3, h=5, w=9, B=2, r=1, grid=(2, 3))


def _bev(Kc, kernel, rot, thr, **kw):
    name = f'bev_kc{Kc}{"_seg3" if kernel == 3 else ""}_rot{rot}_{thr}' + ('_r2' if kw.get('r') == 2 else '')
    assert name not in BEV
    BEV[name] = dict(_BEV_BASE, name=name, family='tie_bev', Kc=Kc, seg_kernel=kernel, rot=rot, thr_name=thr, threshold=THRESHOLDS[thr],
                     head_route='seg3' if kernel == 3 else ('bev_chain' if Kc <= 8 else 'bev_separate'), seed=2500 + len(BEV), **kw)


# bias of class k = BIAS_VALUES[(k + rot) % 3]: over the three rotations every value sits on bit 0 and on bit Kc - 1, and at
# Kc >= 6 every rotation has all three values in both half-waves (bits 4h + e)
for _kc, _kernel in ((1, 1), (6, 1), (8, 1), (9, 1), (32, 1), (6, 3), (9, 3)):
    for _rot in (0, 1, 2):
        for _thr in THRESHOLDS:
            _bev(_kc, _kernel, _rot, _thr)
_bev(8, 1, 1, 'half', r=2)
_bev(9, 1, 2, 'below_half', r=2)


def bev_variants(c):
    """(id, DDPEngine keyword arguments): both engines, and the separate kernels on the <= 8-class cases (DDP_FLAG_UNFUSED_TAIL)"""
    v = [('bf16x3', dict(gemm='bf16x3')), ('f32', dict(gemm='f32'))]
    if c['Kc'] <= 8:
        v.append(('unfused-tail', dict(gemm='bf16x3', fused_tail=False)))
    return v


def bev_pairs():
    return [(n, vid) for n, c in BEV.items() for vid, _ in bev_variants(c)]


def bev_biases(c):
    return torch.tensor([BIAS_VALUES[(k + c['rot']) % 3] for k in range(c['Kc'])])


def bev_state(c):
    sd = synthetic.make_state_dict('bev', c['Kc'], c['L'], c['Cx'], seed=c['seed'], seg_conv_kernel=c['seg_kernel'])
    sd['decode_head.conv_seg.weight'] = torch.zeros_like(sd['decode_head.conv_seg.weight'])
    sd['decode_head.conv_seg.bias'] = bev_biases(c)
    return sd


def bev_expected_bits(c):
    """(Kc,) bool: the classes whose probability exceeds the case's threshold - +8 always, 0 only under the lower threshold"""
    b = bev_biases(c)
    return (b > 0) | ((b == 0) & (c['thr_name'] == 'below_half'))


def bev_engine_kwargs(c):
    return dict(S.engine_kwargs(c), bev_seg_kernel=c['seg_kernel'])


def _bev_cfg(c):
    s = S.bev_scopes(c)
    return dict(randsteps=c['r'], bit_scale=c['bit_scale'], threshold=c['threshold'], num_classes=c['Kc'], timesteps=c['K'],
                time_difference=c['td'], seg_conv_kernel=c['seg_kernel'], input_scope=s['input_scope'], output_scope=s['output_scope'])


_BEV_ORACLE = {}


def bev_oracle(c):
    """-> dict(out (B,Kc,H,W), pred (K,B,r,Kc,H,W) bool): ``O.ddim_sample_bev`` image by image; the per-step thresholded maps - and
    the 3x3 head, which the oracle does not have - from the restatement of tests/bev_head_util.py (the host test pins its output
    to the oracle's, bit for bit, on the 1x1 cases)."""
    import bev_head_util as BU
    if c['name'] in _BEV_ORACLE:
        return _BEV_ORACLE[c['name']]
    sd = bev_state(c)
    x, noise, _ = S.inputs(c)
    outs, preds, restated = [], [], []
    with torch.no_grad():
        for b in range(c['B']):
            trace = []
            o, _ = BU.sample(x[b:b + 1], noise[b], sd, _bev_cfg(c), trace)
            restated.append(o)
            preds.append(torch.stack([t['pred'] for t in trace]))
            outs.append(o if c['seg_kernel'] == 3 else S.oracle_image(c, sd, x, noise, None, b))
    _BEV_ORACLE[c['name']] = dict(out=torch.cat(outs, dim=0), restated=torch.cat(restated, dim=0), pred=torch.stack(preds, dim=1))
    return _BEV_ORACLE[c['name']]
