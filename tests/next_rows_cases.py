"""The geometry sweep of the rows around the sampling loop, shared by tests/test_next_rows_gpu.py (GPU: every case against the
CPU oracle, through guarded workspaces) and tests/test_next_rows_host.py (CPU: conditioning of the oracle, near-tie shares,
route statements, workspace sums).  Imports no GPU.

Four families, each a table of plain dicts with a name, a family, a seed and explicit sizes:

  NECK   ``ddp_neck_fpn`` / ``ddp_neck_fpn_msm`` / ``ddp_neck_msm``.  ``fpn_core`` (csrc/ddp_api.hip) decides per level where the
         GroupNorm sums come from: the stream GEMM's epilogue when ``h * w % 32 == 0`` (k_layer MODE 5, ``gn_partial``), the
         separate kernels otherwise; when all four levels qualify ONE ``k_gn_final32_multi`` launch finalises them.  ``routes``
         states the route of every level ('epilogue' | 'separate') and ``all32`` the one-launch route BY HAND - the host test
         checks the statements against the shapes, so the route a case runs is a property of this table.  (No profiler tag
         covers these launches: there is no launch witness.)  The four (h, w) pairs are explicit: the ABI takes any sizes >= 1.
  FCN    ``ddp_fcn_head_forward``: num_convs 0 .. 8, dilation up to beyond the map, 1 .. 256 classes, maps of one pixel / row /
         column, exactly one tile, one token past a tile, tiles that hold parts of three maps.
  LOOP   ``ddp_sample_fcn``: B > 1 with r > 1, DDPM with B > 1, feature widths other than 256, 0 and 8 convolutions,
         DDP_MAX_STEPS steps.
  EPI    the four post-loop epilogues at DDP_MAX_AUGS / DDP_MAX_WINDOWS, 1 / 2 / 256 classes, one-pixel maps, outputs smaller
         than the map.

Conditioning (tests/test_next_rows_host.py): every neck, head and loop case keeps its fp32 oracle within COND = REL / 20 of
its own fp64 evaluation with the generators' own seeds and input scales - no case needed another seed or scale."""
import ctypes as C

import torch
import torch.nn.functional as F

from config_space_cases import COND, REL  # noqa: F401  (the suite bar and the conditioning rule, not restated)
from ddp_amd import _lib, schedule
from ddp_amd.utils import synthetic
from oracle import ddp_oracle as O
from support import FcnLoop, Guarded, assert_guards, finite, stream

STAGE_BYTES = 48 * 1024        # one stage image of the stream GEMM (b3::LYR_STAGE_B, csrc/layer_bf16x3.h)
MARGIN = 1e-5                  # top-2 margin below which a decision may fall either way (tests/test_hip_parity.py epilogue tests)
TIE_SHARE = 1e-3               # share of such pixels a case may have

SWIN_T = [96, 192, 384, 768]
SWIN_L = [192, 384, 768, 1536]


def _pyramid(h, w):
    return [(-(-h // (1 << l)), -(-w // (1 << l))) for l in range(4)]


# ---- necks ----------------------------------------------------------------------------------------------------------------------
NECK = {}
E, S = 'epilogue', 'separate'


def _neck(name, B, levels, routes, all32, channels=SWIN_T, msm=True, what=''):
    assert name not in NECK
    NECK[name] = dict(name=name, family='neck', seed=900 + len(NECK), B=B, levels=[tuple(x) for x in levels], channels=list(channels),
                      routes=list(routes), all32=all32, msm=msm, what=what)


_neck('all32_min', 2, [(32, 64), (16, 32), (8, 16), (4, 8)], [E, E, E, E], True,
      what='smallest pyramid with every level a multiple of 32; level 3: 64 rows in one tile, level 2 exactly one tile')
_neck('all32_straddle', 3, [(12, 8), (8, 4), (8, 4), (4, 8)], [E, E, E, E], True,
      what='a 256-row tile holds 2 2/3 images of level 0, eight images worth of rows of the others; ratios 1.5, 1, non-integer')
_neck('mixed_low_ragged', 2, [(9, 7), (8, 8), (4, 8), (4, 8)], [S, E, E, E], False,
      what='level 0 on the separate statistics kernels, the rest on the epilogue')
_neck('one_pixel_b1', 1, [(1, 1)] * 4, [S, S, S, S], False, what='single-token levels')
_neck('one_pixel_b2', 2, [(1, 1)] * 4, [S, S, S, S], False, what='single-token levels, two images')
_neck('one_row', 2, [(1, 40), (1, 20), (1, 10), (1, 5)], [S, S, S, S], False, what='one-row levels')
_neck('one_col', 1, [(37, 1), (19, 1), (10, 1), (5, 1)], [S, S, S, S], False, what='one-column levels')
_neck('flat_pyramid', 1, [(13, 19), (5, 7), (5, 7), (2, 2)], [S, S, S, S], False, what='upsample ratio 1 and non-integer ratios')
_neck('chan_min', 2, [(8, 8), (4, 4), (2, 2), (1, 1)], [E, S, S, S], False, channels=[64, 64, 64, 64], msm=False,
      what='the 64-channel limit: two stages per lateral GEMM')
_neck('chan_max', 1, [(8, 8), (4, 4), (2, 2), (1, 1)], [E, S, S, S], False, channels=[4096, 2336, 1536, 64], msm=False,
      what='the 4096-channel limit; two levels wider than the 2304 default of max_w in fpn_layout')
_neck('swin_l', 2, _pyramid(128, 256), [E, E, E, E], True, channels=SWIN_L, msm=False,
      what='Swin-L channels on the pyramid that ENDS at 16 x 32 (128 x 256 ... 16 x 32, the BASELINE shapes): 256 level-0 tiles')
_neck('tiles_gt_cus', 2, _pyramid(192, 192), [E, E, E, E], True,
      what='288 level-0 tiles on 256 CUs: the persistent kernel takes a second tile')
_neck('coarse_larger', 2, [(4, 4), (8, 8), (2, 2), (1, 1)], [S, E, S, S], False,
      what='level 1 larger than level 0: nearest / bilinear DOWN-sampling in the top-down path and the merging')

# ('swin_l': a pyramid that STARTS at 16 x 32 ends at 2 x 4 = 8 tokens and cannot be all-32; the all-32 pyramid with a 16 x 32
# level is the one every BASELINE configuration runs, 128 x 256 ... 16 x 32)


def neck_names(msm_only=False):
    return [n for n, c in NECK.items() if c['msm'] or not msm_only]


def backbone_levels(c):
    """the four backbone-like inputs (B, C_l, h_l, w_l) ~ N(0, 1) of a neck case"""
    g = torch.Generator().manual_seed(70_000 + c['seed'])
    return [torch.randn((c['B'], ch, h, w), generator=g) for ch, (h, w) in zip(c['channels'], c['levels'])]


def fpn_like_levels(c):
    """four 256-channel levels (B, 256, h_l, w_l) ~ N(0, 1): the inputs of MultiStageMerging run alone"""
    g = torch.Generator().manual_seed(30_000 + c['seed'])
    return [torch.randn((c['B'], 256, h, w), generator=g) for h, w in c['levels']]


def fpn_state(c):
    return synthetic.make_fpn_state_dict(c['channels'], c['seed'])


def msm_state(c):
    return synthetic.make_neck_state_dict(c['seed'])


def _cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


_NECK_ORACLE = {}


def neck_oracle(c, dtype=torch.float32, images=None):
    """-> dict(fpn=(4 outputs), chain=merged map (align_corners False), msm={ac: merged map of the 256-channel levels});
    computed once per (case, dtype, images) and process.  ``images``: a slice of the batch (the oracle treats images independently)."""
    key = (c['name'], dtype, images)
    if key not in _NECK_ORACLE:
        sl = slice(None) if images is None else slice(*images)
        sdf, sdm = _cast(fpn_state(c), dtype), _cast(msm_state(c), dtype)
        with torch.no_grad():
            fpn = O.neck_fpn([t[sl].to(dtype) for t in backbone_levels(c)], sdf)
            res = dict(fpn=fpn, chain=O.neck_multi_stage_merging(list(fpn), sdm, False))
            if c['msm']:
                lv = [t[sl].to(dtype) for t in fpn_like_levels(c)]
                res['msm'] = {ac: O.neck_multi_stage_merging(lv, sdm, ac) for ac in (False, True)}
        _NECK_ORACLE[key] = res
    return _NECK_ORACLE[key]


def fpn_level_structs(c, sd):
    """(ddp_fpn_level[4]) of the case; weights from ``sd`` (device tensors for a call, anything for a workspace query)"""
    lv = (_lib.DdpFpnLevel * 4)()
    for l, (ch, (h, w)) in enumerate(zip(c['channels'], c['levels'])):
        lv[l].in_channels, lv[l].h, lv[l].w = ch, h, w
        if sd is not None:
            for f, k in (('lat_w', f'lateral_convs.{l}.conv.weight'), ('lat_gn_w', f'lateral_convs.{l}.gn.weight'),
                         ('lat_gn_b', f'lateral_convs.{l}.gn.bias'), ('out_w', f'fpn_convs.{l}.conv.weight'),
                         ('out_gn_w', f'fpn_convs.{l}.gn.weight'), ('out_gn_b', f'fpn_convs.{l}.gn.bias')):
                setattr(lv[l], f, sd[k].data_ptr())
    return lv


def level_sizes(c):
    return (C.c_int * 4)(*[h for h, _ in c['levels']]), (C.c_int * 4)(*[w for _, w in c['levels']])


def neck_queries(lib, c, B=None):
    """-> (fpn bytes, msm bytes, chain bytes) from the library's own queries"""
    B = c['B'] if B is None else B
    lv = fpn_level_structs(c, None)
    lh, lw = level_sizes(c)
    out = []
    for call in (lambda n: lib.ddp_neck_fpn_workspace(lv, B, C.byref(n)), lambda n: lib.ddp_neck_msm_workspace(B, lh, lw, C.byref(n)),
                 lambda n: lib.ddp_neck_fpn_msm_workspace(lv, B, C.byref(n))):
        n = C.c_size_t(0)
        _lib.check(call(n), lib)
        out.append(n.value)
    return tuple(out)


# ---- FCNHeadWithTime ------------------------------------------------------------------------------------------------------------
FCN = {}


def _fcn(name, num_convs, dilation, classes, maps, h, w, bn, time):
    assert name not in FCN
    FCN[name] = dict(name=name, family='fcn', seed=950 + len(FCN), num_convs=num_convs, dilation=dilation, classes=classes, maps=maps,
                     h=h, w=w, bn=bn, time=time)


#     name             convs dil  cls  maps h   w    BN     time
_fcn('5x7_d1',          3,   1,   32,  2,  5,  7,   True,  True)
_fcn('5x7_d3',          2,   3,   33,  2,  5,  7,   False, True)
_fcn('5x7_d16',         2,   16,  19,  2,  5,  7,   True,  True)      # only the centre tap is inside the map
_fcn('pixel_d3',        3,   3,   1,   1,  1,  1,   True,  False)
_fcn('pixel_d16',       1,   16,  256, 1,  1,  1,   False, True)
_fcn('row_d3',          2,   3,   255, 2,  1,  37,  True,  True)
_fcn('row_d16',         1,   16,  32,  2,  1,  37,  False, False)
_fcn('col_d3',          1,   3,   33,  2,  37, 1,   False, True)
_fcn('col_d16',         2,   16,  1,   2,  37, 1,   True,  True)
_fcn('m256_d3',         8,   3,   150, 1,  16, 16,  True,  True)      # M = 256: exactly one tile
_fcn('m256_d16',        1,   16,  256, 1,  16, 16,  True,  False)
_fcn('m257_d3',         1,   3,   19,  1,  1,  257, False, True)      # one token past a tile
_fcn('m257_d16',        3,   16,  255, 1,  1,  257, True,  True)
_fcn('three_maps_d3',   2,   3,   19,  3,  10, 10,  True,  True)      # tiles hold parts of three maps
_fcn('three_maps_d16',  1,   16,  33,  3,  10, 10,  False, False)
_fcn('no_convs',        0,   1,   19,  2,  5,  7,   True,  True)      # conv_seg alone
_fcn('no_convs_k256',   0,   1,   256, 1,  1,  257, False, False)
_fcn('eight_convs',     8,   1,   32,  3,  10, 10,  False, True)
_fcn('one_class',       1,   1,   1,   3,  10, 10,  True,  False)


def fcn_state(c):
    return synthetic.make_fcn_state_dict(c['num_convs'], c['classes'], c['bn'], False, c['seed'])


def fcn_inputs(c):
    feat, temb = synthetic.make_fcn_inputs(c['maps'], c['h'], c['w'], c['seed'])
    return feat, (temb if c['time'] else None)


def centre_tap_only(sd):
    """the same head with every off-centre tap of its 3x3 convolutions zeroed"""
    out = dict(sd)
    for k, v in sd.items():
        if k.startswith('convs.') and k.endswith('conv.weight'):
            z = torch.zeros_like(v)
            z[:, :, 1, 1] = v[:, :, 1, 1]
            out[k] = z
    return out


_FCN_ORACLE = {}


def fcn_oracle(c, dtype=torch.float32, centre=False):
    key = (c['name'], dtype, centre)
    if key not in _FCN_ORACLE:
        sd = fcn_state(c)
        sd = _cast(centre_tap_only(sd) if centre else sd, dtype)
        feat, temb = fcn_inputs(c)
        with torch.no_grad():
            _FCN_ORACLE[key] = O.fcn_head_forward(feat.to(dtype), temb.to(dtype) if temb is not None else None, sd, c['num_convs'],
                                                  1 if centre else c['dilation'])
    return _FCN_ORACLE[key]


def fcn_query(lib, c, maps=None):
    n = C.c_size_t(0)
    _lib.check(lib.ddp_fcn_head_workspace(c['maps'] if maps is None else maps, c['h'], c['w'], c['classes'], C.byref(n)), lib)
    return n.value


# ---- sampler loop around the FCN head -------------------------------------------------------------------------------------------
LOOP = {}


def _loop(name, **kw):
    c = dict(name=name, family='loop', seed=980 + len(LOOP), B=2, r=1, K=3, sampler='ddim', classes=19, h=6, w=9, Cx=256, num_convs=2,
             dilation=1, bn=True, accumulation=True, bit_scale=0.01, td=1)
    c.update(kw)
    assert name not in LOOP
    LOOP[name] = c


_loop('b2_r2_ddim', r=2)
_loop('b3_ddpm_k150', B=3, sampler='ddpm', classes=150, h=5, w=11, bn=False)
_loop('b2_r2_ddpm', r=2, sampler='ddpm', accumulation=False)
_loop('cx64', Cx=64, h=5, w=7)
_loop('cx512', Cx=512, h=5, w=7, r=2, dilation=2)
_loop('no_convs', num_convs=0, h=5, w=7)
_loop('eight_convs', num_convs=8, h=5, w=7, bn=False)
_loop('max_steps', K=_lib.MAX_STEPS, num_convs=1, h=3, w=4)          # conv_streams: timesteps x convs x 72 stages


def loop_state(c):
    """hot-path state_dict of DDP(decode_head=FCNHeadWithTime) with a transform conv over Cx + 256 channels"""
    sd = {k: v for k, v in synthetic.make_state_dict('seg', c['classes'], 0, c['Cx'], seed=c['seed']).items()
          if not k.startswith('decode_head.')}
    sd.update({'decode_head.' + k: v
               for k, v in synthetic.make_fcn_state_dict(c['num_convs'], c['classes'], c['bn'], False, c['seed']).items()})
    return sd


def loop_inputs(c):
    """-> x (B,Cx,h,w), noise (B,r,256,h,w), step_noise (K,B,r,256,h,w) or None"""
    x, noise = synthetic.make_inputs(c['B'], c['h'], c['w'], c['r'], c['Cx'], 256, seed=c['seed'] + 1)
    sn = None
    if c['sampler'] == 'ddpm':
        g = torch.Generator().manual_seed(c['seed'] + 2)
        sn = torch.randn((c['K'], c['B'], c['r'], 256, c['h'], c['w']), generator=g)
    return x, noise, sn


def loop_cfg(c, gemm='bf16x3', batch=None, flags=0):
    cfg = _lib.DdpCfg()
    cfg.abi_version = _lib.ABI_VERSION
    cfg.task = _lib.TASK_SEG
    cfg.sampler = _lib.SAMPLER_DDPM if c['sampler'] == 'ddpm' else _lib.SAMPLER_DDIM
    cfg.batch, cfg.randsteps, cfg.timesteps, cfg.num_layers = (c['B'] if batch is None else batch), c['r'], c['K'], 0
    cfg.num_classes, cfg.feat_channels = c['classes'], c['Cx']
    cfg.h = cfg.head_h = c['h']
    cfg.w = cfg.head_w = c['w']
    cfg.accumulation, cfg.bit_scale = int(bool(c['accumulation'])), c['bit_scale']
    cfg.gemm_mode = _lib.GEMM_BF16X3 if gemm == 'bf16x3' else _lib.GEMM_F32_MFMA
    cfg.flags = flags
    return cfg


def loop_steps(c):
    recs = schedule.step_records('seg', c['K'], c['td'], 0.0, 'cosine', c['sampler'])
    steps = (_lib.DdpStep * c['K'])()
    for i, r in enumerate(recs):
        for k, v in r.items():
            setattr(steps[i], k, v)
    return steps


def loop_query(lib, c, gemm='bf16x3', batch=None):
    n = C.c_size_t(0)
    cfg = loop_cfg(c, gemm, batch)
    _lib.check(lib.ddp_sample_fcn_workspace(C.byref(cfg), c['num_convs'], c['dilation'], C.byref(n)), lib)
    return n.value


_LOOP_ORACLE = {}


def loop_oracle(c, dtype=torch.float32):
    """(B, classes, h, w): the reference sampler around the reference FCN head, one image per run"""
    key = (c['name'], dtype)
    if key not in _LOOP_ORACLE:
        sd = _cast(loop_state(c), dtype)
        x, noise, sn = loop_inputs(c)
        head = O.fcn_head_for_sampler(sd, c['num_convs'], c['dilation'])
        kw = dict(timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'], time_difference=c['td'], accumulation=c['accumulation'],
                  head=head)
        outs = []
        with torch.no_grad():
            for b in range(c['B']):
                xb, nb = x[b:b + 1].to(dtype), noise[b].to(dtype)
                if c['sampler'] == 'ddpm':
                    outs.append(O.ddpm_sample_seg(xb, nb, sn[:, b].to(dtype), sd, **kw))
                else:
                    outs.append(O.ddim_sample_seg(xb, nb, sd, **kw))
        _LOOP_ORACLE[key] = torch.cat(outs, dim=0)
    return _LOOP_ORACLE[key]


def top2_margin(p):
    """(B, K, ...) scores or probabilities -> (B, ...) margin between the two largest; one class: no decision to lose"""
    if p.shape[1] < 2:
        return torch.full_like(p[:, 0], float('inf'))
    t = p.topk(2, dim=1).values
    return t[:, 0] - t[:, 1]


# ---- post-loop epilogues --------------------------------------------------------------------------------------------------------
EPI = {}


def _epi(name, kind, **kw):
    assert name not in EPI
    EPI[name] = dict(name=name, family='epilogue', kind=kind, seed=1000 + len(EPI), **kw)


_epi('post_pixel_to_7x5', 'post', B=2, K=19, h=1, w=1, img=(7, 5), crop=None, out=None, align=False, flip=None)
_epi('post_shrink', 'post', B=2, K=19, h=24, w=32, img=(9, 11), crop=None, out=None, align=False, flip=None)
_epi('post_shrink_two_stage', 'post', B=2, K=19, h=24, w=32, img=(48, 64), crop=(40, 60), out=(9, 11), align=False, flip='horizontal')
for _k in (1, 2, 256):
    _epi(f'post_k{_k}', 'post', B=2, K=_k, h=6, w=10, img=(24, 40), crop=(21, 37), out=(30, 50), align=False, flip=None)
_epi('post_k256_x4', 'post', B=2, K=256, h=6, w=10, img=(24, 40), crop=None, out=None, align=False, flip='vertical')
for _ac in (False, True):
    for _fl in (None, 'horizontal', 'vertical'):
        _epi(f'post_b3_ac{int(_ac)}_{_fl or "noflip"}', 'post', B=3, K=19, h=7, w=9, img=(28, 36), crop=(25, 33), out=(31, 40), align=_ac,
             flip=_fl)
# exactly DDP_MAX_AUGS augmentations: four map sizes, image = 4 x map, crops and flips mixed
_epi('aug_16', 'aug', B=2, K=19, out=(20, 30), align=False,
     augs=[dict(h=3 + i % 4, w=5 + (i // 2) % 4, crop_cut=(i % 3, (i + 1) % 3), flip=(None, 'horizontal', 'vertical')[i % 3])
           for i in range(_lib.MAX_AUGS)])
# exactly DDP_MAX_WINDOWS windows: an 8 x 8 grid of 4 x 4 windows at stride 2 on an 18 x 18 image, window maps of 2 x 3
_epi('slide_64', 'slide', B=2, K=19, h=2, w=3, img=(18, 18), crop_size=(4, 4), stride=(2, 2), keep=(17, 16), out=(20, 23), align=False,
     flip='horizontal')
_epi('depth_16', 'depth', B=2, out=(12, 18), align=False,
     augs=[dict(h=3 + i % 5, w=4 + (i // 3) % 4, flip=(None, 'horizontal', 'vertical')[i % 3]) for i in range(_lib.MAX_AUGS)])
_epi('depth_pixel', 'depth', B=2, out=(5, 7), align=True, augs=[dict(h=1, w=1, flip=None), dict(h=1, w=1, flip='vertical')])
_epi('depth_one_wide', 'depth', B=2, out=(9, 1), align=False, augs=[dict(h=6, w=4, flip='horizontal'), dict(h=3, w=1, flip=None)])
MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0


def epi_names(kind):
    return [n for n, c in EPI.items() if c['kind'] == kind]


def post_scores(c):
    return synthetic.make_scores(c['B'], c['K'], c['h'], c['w'], c['seed'])


def post_probs(c, scores):
    """the probabilities whose argmax ``oracle.seg_postprocess`` returns (its op sequence up to the argmax; the host test pins
    the argmax of this to the oracle's class map)"""
    o = F.interpolate(scores, size=tuple(c['img']), mode='bilinear', align_corners=c['align'])
    if c['crop'] is not None:
        o = o[:, :, :c['crop'][0], :c['crop'][1]]
        o = F.interpolate(o, size=tuple(c['out'] if c['out'] is not None else c['crop']), mode='bilinear', align_corners=c['align'])
    o = F.softmax(o, dim=1)
    if c['flip'] == 'horizontal':
        o = o.flip(dims=(3,))
    elif c['flip'] == 'vertical':
        o = o.flip(dims=(2,))
    return o


def aug_inputs(c):
    """-> (scores list, metas) of an 'aug' case: network input 4 x the map, cropped by crop_cut"""
    scores, metas = [], []
    for i, a in enumerate(c['augs']):
        scores.append(synthetic.make_scores(c['B'], c['K'], a['h'], a['w'], c['seed'] * 100 + i))
        H, W = 4 * a['h'], 4 * a['w']
        metas.append(dict(img_size=(H, W), crop_size=(H - a['crop_cut'][0], W - a['crop_cut'][1]), flip=a['flip']))
    return scores, metas


def slide_grid(c):
    """the window grid of slide_inference (encoder_decoder.py:186-206), restated: -> (ys, xs, crop)"""
    (H, W), (hc, wc), (hs, ws) = c['img'], c['crop_size'], c['stride']
    ys = [max(min(i * hs + hc, H) - hc, 0) for i in range(max(H - hc + hs - 1, 0) // hs + 1)]
    xs = [max(min(j * ws + wc, W) - wc, 0) for j in range(max(W - wc + ws - 1, 0) // ws + 1)]
    return ys, xs, (min(hc, H), min(wc, W))


def slide_inputs(c):
    ys, xs, _ = slide_grid(c)
    return [synthetic.make_scores(c['B'], c['K'], c['h'], c['w'], c['seed'] * 100 + i) for i in range(len(ys) * len(xs))]


def slide_oracle(c):
    """-> (window-averaged scores, probabilities with the flip applied) of a 'slide' case"""
    ys, xs, crop = slide_grid(c)
    raw = O.seg_slide_inference(slide_inputs(c), ys, xs, crop, c['img'], c['keep'], c['out'], c['align'])
    p = torch.softmax(raw, dim=1)
    if c['flip']:
        p = p.flip(dims=(3,) if c['flip'] == 'horizontal' else (2,))
    return raw, p


def depth_inputs(c):
    maps = [synthetic.make_depth_map(c['B'], a['h'], a['w'], c['seed'] * 100 + i) for i, a in enumerate(c['augs'])]
    return maps, [a['flip'] for a in c['augs']]


# ---- device runners: the workspace-taking entries through the C ABI, each on a guarded workspace of exactly the queried size ------
# (tests/test_next_rows_gpu.py; tests/test_workspace_history_gpu.py runs the same entries under other workspace histories)
NECK_DEV = {}


def neck_dev(c, dev):
    """device copies of a neck case's weights and inputs (made once per case)"""
    if c['name'] not in NECK_DEV:
        NECK_DEV.clear()                     # one case at a time: tiles_gt_cus and swin_l hold tens of MB
        sdf = {k: v.to(dev).contiguous() for k, v in fpn_state(c).items()}
        sdm = {k: v.to(dev).contiguous() for k, v in msm_state(c).items()}
        sdm['w'] = sdm['down.conv.weight'].reshape(256, 1024).contiguous()
        NECK_DEV[c['name']] = (sdf, sdm, [t.to(dev) for t in backbone_levels(c)],
                               [t.to(dev) for t in fpn_like_levels(c)] if c['msm'] else None)
    return NECK_DEV[c['name']]


def images(ts, b):
    return ts if b is None else [t[b:b + 1].contiguous() for t in ts]


def run_fpn(c, dev, sdf, xs, flags=0, g=None, what=''):
    """ddp_neck_fpn on a guarded workspace of exactly the queried size -> (four NCHW outputs, the workspace)"""
    lib = _lib.load()
    B = xs[0].shape[0]
    lv = fpn_level_structs(c, sdf)
    g = g or Guarded(neck_queries(lib, c, B)[0], dev)
    outs = [torch.full((B, 256, h, w), float('nan'), device=dev) for h, w in c['levels']]
    pin = (C.c_void_p * 4)(*[x.data_ptr() for x in xs])
    pout = (C.c_void_p * 4)(*[o.data_ptr() for o in outs])
    _lib.check(lib.ddp_neck_fpn(lv, B, pin, pout, flags, g.ptr(), stream(dev)), lib)
    torch.cuda.synchronize()
    assert_guards(g, f'fpn {c["name"]} {what}')
    for l, o in enumerate(outs):
        finite(o, f'fpn {c["name"]} level {l} {what}')
    return outs, g


def run_msm(c, dev, sdm, lvls, align, flags=0, g=None, what=''):
    lib = _lib.load()
    B = lvls[0].shape[0]
    lh, lw = level_sizes(c)
    g = g or Guarded(neck_queries(lib, c, B)[1], dev)
    out = torch.full((B, 256) + c['levels'][0], float('nan'), device=dev)
    ptrs = (C.c_void_p * 4)(*[t.data_ptr() for t in lvls])
    _lib.check(lib.ddp_neck_msm(ptrs, lh, lw, B, sdm['w'].data_ptr(), sdm['down.gn.weight'].data_ptr(), sdm['down.gn.bias'].data_ptr(),
                                int(align), flags, out.data_ptr(), g.ptr(), stream(dev)), lib)
    torch.cuda.synchronize()
    assert_guards(g, f'msm {c["name"]} {what}')
    finite(out, f'msm {c["name"]} {what}')
    return out, g


def run_chain(c, dev, sdf, sdm, xs, align=False, flags=0, g=None, what=''):
    lib = _lib.load()
    B = xs[0].shape[0]
    lv = fpn_level_structs(c, sdf)
    g = g or Guarded(neck_queries(lib, c, B)[2], dev)
    out = torch.full((B, 256) + c['levels'][0], float('nan'), device=dev)
    pin = (C.c_void_p * 4)(*[x.data_ptr() for x in xs])
    _lib.check(lib.ddp_neck_fpn_msm(lv, B, pin, sdm['w'].data_ptr(), sdm['down.gn.weight'].data_ptr(), sdm['down.gn.bias'].data_ptr(),
                                    int(align), flags, out.data_ptr(), g.ptr(), stream(dev)), lib)
    torch.cuda.synchronize()
    assert_guards(g, f'chain {c["name"]} {what}')
    finite(out, f'chain {c["name"]} {what}')
    return out, g


def fcn_head(c, sd, dev):
    import ddp_amd
    head = ddp_amd.FCNHeadWithTime(num_convs=c['num_convs'], kernel_size=3, concat_input=False, dilation=c['dilation'], in_channels=256,
                                   channels=256, num_classes=c['classes'], in_index=0, norm_cfg=dict(type='BN') if c['bn'] else None)
    head.load_state_dict(sd, strict=True)
    return head.to(dev).eval()


def device_loop(c, dev, gemm='bf16x3', batch=None):
    """ddp_prepare_fcn / ddp_sample_fcn through the C ABI for a LOOP case (ddp_amd.engine.FcnSamplerEngine fixes 256 feature
    channels; the C ABI takes any multiple of 32)"""
    B = c['B'] if batch is None else batch
    sd = loop_state(c)
    head = fcn_head(dict(c, maps=1), {k[len('decode_head.'):]: v for k, v in sd.items() if k.startswith('decode_head.')}, dev)
    loop = FcnLoop(c, sd, dev, B, head.conv_array(), loop_cfg(c, gemm, B), loop_steps(c), loop_query(_lib.load(), c, gemm, B), 'loop')
    loop.head = head
    return loop
