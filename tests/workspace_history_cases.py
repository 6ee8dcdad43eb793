"""Targets, fills and polluters shared by tests/test_workspace_history_gpu.py (GPU) and tests/test_workspace_history_host.py (CPU).

The property under test needs no tolerance: the bits of every output of a call are a function of its arguments and of the
caller-written regions only - not of the bytes the workspace held before, not of the calls that ran before.  The oracle comparisons
of the suite all have the same history (a fresh engine, a workspace filled with the quiet NaN 0x7FC0BEEF, the first call), and the
decision and clamp kernels swallow a NaN (tests/test_workspace_history_host.py shows the arithmetic), so neither a read of
uninitialised workspace nor stale finite state of an earlier call is visible there.

A TARGET is one case that already has an oracle expectation in the suite, at its existing shape, with the route table of the file it
was taken from; nothing is copied: the case dicts, state dicts, inputs, maps and expectations are the sibling modules' own objects.
  config_space_cases      the smallest-work case of every ``path`` (two steps or more, no one-row / one-pixel map) and, by name, the
                          rows of the table the path key does not separate: seg DDPM, depth with r > 1, L = 1, one-row and one-pixel
                          depth, a feature width other than 256 (the seg_prologue pick is one)
  x0_hint_cases           partial hints, seg and depth            prior_start_cases   seg / depth / bev from the case's own t_start
  class_prior_cases       the soft rows                           score_prior_cases   the soft map; soft map + class rows ('both')
  ddpm_chain_cases        DDP_FLAG_DDPM_CHAIN                     seeded_noise_util   step record + seeded noise
  test_workspace_regions_gpu   every conditioning flag in one engine (B = 2, r = 2, h = 3, w = 5)
FCN-head loops (``ddp_sample_fcn``) and the stand-alone entries are listed in LOOPS and ENTRIES.

FILLS are 32-bit words written over the interior of the guarded buffer (the two 4 KiB guards keep the suite's PATTERN, so the
existing ``_assert_guards`` checks them).  POLLUTERS are calls made on the SAME engine in front of the target call."""
import ctypes as C

import torch

import class_prior_cases as PC
import config_space_cases as S
import ddpm_chain_cases as D
import fcn_gn_cases as G
import next_rows_cases as N
import prior_start_cases as PS
import score_prior_cases as SP
import seeded_noise_util as U
import x0_hint_cases as H
from ddp_amd import _lib
from ddp_amd.utils import synthetic
from golden_util import max_rel
from support import PATTERN, REL

FILLS = {'nan': PATTERN,              # the suite's quiet NaN
         'zero': 0x00000000,
         'one': 0x3F800000,           # 1.0, a plausible activation
         'inf': 0x7F800000,
         'neg_flt_max': 0xFF7FFFFF,
         'x41': 0x41414141}           # 12.08 as float; as bytes a class id of 65 and a valid depth
HISTORY_FILLS = ('nan', 'zero')       # the history tests run on both: see test_history_independence
POLLUTERS = ('other_inputs', 'nan_inputs', 'bigger_then_back', 'smaller_then_back', 'other_batch')
NAN_INPUT_ROUTES = ('bf16x3', 'f32', 'unfused-layer')      # + the bf16x3 route of the seg ddpm case: test_nan_input_does_not_fault's four


def i32(word):
    """a 32-bit word as the signed value torch's int32 holds"""
    return word - (1 << 32) if word >= (1 << 31) else word


def decisions_agree(c, out, ref):
    d, dr = S.decisions(c, out), S.decisions(c, ref)
    return 1.0 if d is None else float((d == dr).float().mean())


class Target:
    """One sampler case with its routes.  ``c``: the case dict (config_space_cases keys); ``routes``: {id: (gemm, flags)} of the
    source file; ``ekw``: the engine keywords the family adds; ``seed``: the key of a seeded engine (None: the case's noise)."""

    def __init__(self, tid, source, path, c, routes, ekw=None, seed=None, state=S.state_dict, engine_kwargs=S.engine_kwargs):
        self.id, self.source, self.path, self.c, self.ekw, self.seed = tid, source, path, c, dict(ekw or {}), seed
        self.routes = {vid: (gemm, dict(fl)) for vid, gemm, fl in routes}
        self._state, self._engine_kwargs = state, engine_kwargs

    def state_dict(self):
        return self._state(self.c)

    def engine_kwargs(self):
        return self._engine_kwargs(self.c)

    def geometry(self):
        return self.c['B'], self.c['h'], self.c['w']

    def inputs(self):
        """-> dict(x, noise, sn, seed, regions) of the target call: the case's own tensors"""
        x, noise, sn = S.inputs(self.c)
        if self.seed is not None:
            noise = sn = None
        return dict(x=x, noise=noise, sn=sn, seed=self.seed, regions=self.regions())

    def regions(self):
        """{region: CPU tensor} the case writes; a region the engine has and the case does not name is cleared"""
        return {}

    def expectation(self):
        """the cached oracle expectation (loaded by the CPU companion); None: formed from the call's own start noise on the GPU"""
        return None

    def check(self, o, label):
        raise NotImplementedError

    # ---- polluters ------------------------------------------------------------------------------------------------------------
    def polluter_geometry(self, name):
        B, h, w = self.geometry()
        return {'bigger_then_back': (B + 1, 2 * h + 1, 2 * w + 3), 'smaller_then_back': (1, max(1, h - 2), max(1, w - 3)),
                'other_batch': (1, h, w)}[name]

    def polluters(self, vid):
        c = self.c
        out = ['other_inputs', 'bigger_then_back', 'smaller_then_back']
        seg_plain = c['task'] == 'seg' and self.source == 'config_space_cases'
        if seg_plain and (vid in NAN_INPUT_ROUTES if c['sampler'] == 'ddim' else vid == 'bf16x3'):
            out.append('nan_inputs')
        if c['B'] > 1:
            out.append('other_batch')
        return out

    def inputs_at(self, geometry, nan=False):
        """deterministic inputs of another seed at ``geometry``: x and the start noise scaled by 1e3 (hostile_stats_cases x_1e3 /
        noise_1e3), every caller region dense and different, another key for a seeded engine; ``nan``: NaN and +-inf planted"""
        c = self.c
        B, h, w = geometry
        cm = 1 if c['task'] == 'depth' else 256
        seed = c['seed'] + 5000 + 7 * B + 3 * h + w
        x, noise = synthetic.make_inputs(B, h, w, c['r'], c['Cx'], cm, seed=seed)
        x, noise = x * 1e3, noise * 1e3
        g = torch.Generator().manual_seed(seed + 1)
        sn = torch.randn((c['K'], B, c['r'], cm, h, w), generator=g) if c.get('sampler') == 'ddpm' else None
        if nan:
            x[0, :, h // 2, w // 2] = float('nan')
            x[0, min(5, c['Cx'] - 1), 0, 0] = float('inf')
            noise[B - 1, 0, :, h - 1, w - 1] = float('nan')
            noise[0, 0, 0, 0, 0] = float('-inf')
        kc = c['Kc']
        regions = {}
        if c['task'] == 'seg':
            regions['hints'] = torch.randint(0, kc, (B, h, w), generator=g).to(torch.uint8)           # all pixels hinted
            regions['prior'] = torch.randint(0, kc, (B, h, w), generator=g).to(torch.uint8)           # a full prior map
            rows = 3.0 * torch.randn((B, kc), generator=g)
            if kc > 1:
                rows[:, 1::3] = float('-inf')                                                            # -inf rows; class 0 stays in
            regions['class_prior'] = rows
            regions['score_prior'] = 2.0 * torch.randn((B, kc, h, w), generator=g) + 0.5
        elif c['task'] == 'depth':
            lo, hi = c['min_depth'], c['max_depth']
            regions['hints'] = lo + (hi - lo) * torch.rand((B, h, w), generator=g)
            regions['prior'] = lo + (hi - lo) * torch.rand((B, h, w), generator=g)
        else:
            regions['prior'] = torch.randint(0, 1 << kc, (B, h, w), generator=g).to(torch.int32)
        if self.seed is not None:
            noise = sn = None
        return dict(x=x, noise=noise, sn=sn, seed=None if self.seed is None else self.seed + 1 + seed, regions=regions)


class _Plain(Target):
    def expectation(self):
        return S.oracle_batch(self.c)

    def check(self, o, label):
        S.check_against_oracle(self.c, o['out'], label)


class _Chain(Target):
    def expectation(self):
        return D.oracle_batch(self.c)

    def check(self, o, label):
        D.check_against_oracle(self.c, o['out'], label)


class _Hints(Target):
    def regions(self):
        return dict(hints=H.partial_hints(self.c))

    def expectation(self):
        return H.expected(self.c, 'partial')

    def check(self, o, label):
        want, rec = self.expectation()
        err, agree = H.max_rel(o['out'], want), decisions_agree(self.c, o['out'], want)
        line = f'WS-HISTORY oracle {label}: max-rel {err:.3e} (bar {REL:.0e}), decisions equal {agree:.4f}'
        if self.c['task'] == 'depth':
            e_rec = H.max_rel(o['step_record'], rec)
            line += f', step record {e_rec:.3e}'
            assert e_rec < REL, line
        print(line)
        assert torch.isfinite(o['out']).all() and err < REL and agree > 0.999, line


class _Prior(Target):
    def regions(self):
        return dict(prior=PS.prior(self.c, 0))

    def expectation(self):
        return PS.expected(self.c, 0)

    def check(self, o, label):
        want, _ = self.expectation()
        err, agree = PS.max_rel(o['out'], want), decisions_agree(self.c, o['out'], want)
        print(f'WS-HISTORY oracle {label}: max-rel {err:.3e} (bar {REL:.0e}), decisions equal {agree:.4f}')
        assert torch.isfinite(o['out']).all() and err < REL and agree > 0.999


class _ClassPrior(Target):
    def regions(self):
        return dict(class_prior=PC.rows(self.c, 'soft'))

    def expectation(self):
        return PC.expected(self.c, 'soft')

    def check(self, o, label):
        e = self.expectation()
        err = PC.rel_live(o['out'], e['out'], PC.rows(self.c, 'soft'))
        agree = float((o['step_record'] == e['record']).float().mean())
        print(f'WS-HISTORY oracle {label}: max-rel {err:.3e} (bar {REL:.0e}), decisions equal {agree:.4f} at every step')
        assert torch.isfinite(o['out']).all() and err < REL and agree > 0.999


class _ScorePrior(Target):
    kind = 'soft'

    def regions(self):
        r = dict(score_prior=SP.prior_map(self.c, 'soft'))
        if self.kind == 'both':
            r['class_prior'] = SP.const_rows(self.c)
        return r

    def expectation(self):
        return SP.expected(self.c, self.kind)

    def check(self, o, label):
        e = self.expectation()
        if self.kind == 'both':
            err = SP.max_rel(o['out'], e['out'])
        else:
            err = SP.rel_live(o['out'], e['out'], SP.prior_map(self.c, 'soft'))
        agree = float((o['step_record'] == e['record']).float().mean())
        print(f'WS-HISTORY oracle {label}: max-rel {err:.3e} (bar {REL:.0e}), decisions equal {agree:.4f} at every step')
        assert torch.isfinite(o['out']).all() and err < REL and agree > 0.999


class _BothPriors(_ScorePrior):
    kind = 'both'


class _OwnNoise(Target):
    """seeded engines (and the all-flags engine, whose start map is the seeded noise mixed with a cleared prior at t_start = 1): the
    expectation is ``config_space_cases.oracle_image`` on the start noise the call itself reports, as
    test_seeded_call_equals_unseeded_call_fed_the_generated_noise feeds it back"""
    start = 'last_noise'
    _cache = {}

    def check(self, o, label):
        c = self.c
        noise = o[self.start]
        key = (self.id, noise.numpy().tobytes())
        if key not in self._cache:
            sd, x = self.state_dict(), S.inputs(c)[0]
            self._cache[key] = torch.cat([S.oracle_image(c, sd, x, noise, None, b) for b in range(c['B'])], dim=0)
        ref = self._cache[key]
        errs = [max_rel(o['out'][b:b + 1], ref[b:b + 1]) for b in range(c['B'])]
        agree = decisions_agree(c, o['out'], ref)
        print(f'WS-HISTORY oracle {label}: max-rel per image {" ".join(f"{e:.3e}" for e in errs)} (bar {REL:.0e}), decisions equal {agree:.4f}')
        assert torch.isfinite(o['out']).all() and max(errs) < REL and agree > 0.999


class _AllFlags(_OwnNoise):
    start = 'last_start'


def _work(c):
    return c['B'] * c['r'] * c['h'] * c['w'] * c['K'] * c['L']


def smallest_per_path():
    """{path: case name}: the smallest-work case of every config_space path among those with two steps or more (a one-step call never
    runs an update kernel) and a map of at least two rows and columns (the one-row / one-pixel maps are targets of their own)"""
    best = {}
    for n, c in S.CASES.items():
        if 'path' in c and c['K'] >= 2 and min(c['h'], c['w']) > 1 and (c['path'] not in best or _work(c) < _work(S.CASES[best[c['path']]])):
            best[c['path']] = n
    return best


# the rows of the issue's table the path key does not separate: (row, case)
BY_NAME = [('seg_ddpm', 'seg_ddpm_acc'), ('depth_r2', 'depth_9x11_L2_r2'), ('depth_L1', 'depth_9x11_L1_no_eps'),
           ('depth_one_row', 'depth_1x37_L3'), ('depth_one_pixel', 'depth_1x1_L2')]

TARGETS = {}


def _put(t):
    assert t.id not in TARGETS
    TARGETS[t.id] = t


for _path, _n in sorted(smallest_per_path().items()):
    _put(_Plain('cs-' + _n, 'config_space_cases', _path, S.CASES[_n], S.variants(S.CASES[_n])))
for _row, _n in BY_NAME:
    _put(_Plain('cs-' + _n, 'config_space_cases', _row, S.CASES[_n], S.variants(S.CASES[_n])))
for _n in ('seg_kc19_7x13', 'depth_9x14'):
    _c = H.CASES[_n]
    _put(_Hints('x0-' + _n, 'x0_hint_cases', 'x0_hints_' + _c['task'], _c, H.routes(_c),
                dict(x0_hints=True, **(dict(record_x0=True) if _c['task'] == 'seg' else dict(record_steps=True)))))
for _n in ('seg_kc19_7x13', 'depth_5x10_r2', 'bev_kc8_r1'):
    _c = PS.CASES[_n]
    _put(_Prior('ps-' + _n, 'prior_start_cases', 'prior_start_' + _c['task'], _c, PS.routes(_c),
                dict(prior_start=True, t_start=_c['t_start'], **(dict(record_x0=True) if _c['task'] == 'seg' else {})), state=PS.state_dict))
_c = PC.seeded(PC.CASES['kc19_8x12_b2'], 'soft')
_put(_ClassPrior('cp-kc19_8x12_b2', 'class_prior_cases', 'class_prior', _c, PC.routes(_c), dict(class_prior=True, record_steps=True)))
_c = SP.seeded(SP.CASES['kc19_8x12_b2'], 'soft')
_put(_ScorePrior('sp-kc19_8x12_b2', 'score_prior_cases', 'score_prior', _c, SP.routes(_c), dict(score_prior=True, record_steps=True)))
_c = SP.seeded(SP.CASES['kc19_7x13_b3'], 'both')
_put(_BothPriors('sp-both-kc19_7x13_b3', 'score_prior_cases', 'score_and_class_prior', _c,
                 [r for r in SP.routes(_c) if r[0] in ('bf16x3', 'f32', 'unfused-layer', 'unfused-tail')],     # test_both_priors_add's
                 dict(score_prior=True, class_prior=True, record_steps=True)))
_c = D.ALL['dc_15tok']
_put(_Chain('dc-dc_15tok', 'ddpm_chain_cases', 'ddpm_chain', _c, [(v, 'bf16x3', fl) for v, fl in sorted(D.VIDS.items())],
            dict(ddpm_chain=True), engine_kwargs=D.engine_kwargs))
for _n in ('seg_fused', 'depth_chain_1x37'):
    _c, _fl = U.CASES[_n]
    _fl = dict(_fl)
    _put(_OwnNoise('sn-' + _n, 'seeded_noise_util', 'step_record_seeded_' + _c['task'], _c, [(_n, _fl.pop('gemm', 'bf16x3'), _fl)],
                   dict(seeded_noise=True, record_steps=True), seed=U.SEED))
for _task, _c in S.REGION_CASES.items():
    _put(_AllFlags('all-' + _task, 'test_workspace_regions_gpu', 'all_flags_' + _task, _c, [('bf16x3', 'bf16x3', {})],
                   dict(record_steps=True, seeded_noise=True, x0_hints=True, prior_start=True, class_prior=_task == 'seg'), seed=2024))

ROUTE_TABLES = {'config_space_cases': lambda t: {(v, g) for v, g, _ in S.variants(t.c)},
                'x0_hint_cases': lambda t: {(v, g) for v, g, _ in H.routes(t.c)},
                'prior_start_cases': lambda t: {(v, g) for v, g, _ in PS.routes(t.c)},
                'class_prior_cases': lambda t: {(v, g) for v, g, _ in PC.routes(t.c)},
                'score_prior_cases': lambda t: {(v, g) for v, g, _ in SP.routes(t.c)},
                'ddpm_chain_cases': lambda t: {(v, 'bf16x3') for v in D.VIDS},
                'seeded_noise_util': lambda t: {(n, fl.get('gemm', 'bf16x3')) for n, (_, fl) in U.CASES.items()},
                'test_workspace_regions_gpu': lambda t: {('bf16x3', 'bf16x3')}}

# (path, route) pairs that must appear among the collected ids (tests/test_workspace_history_host.py)
REQUIRED = [('seg_head7', 'bf16x3'), ('seg_head7', 'f32'), ('seg_head7', 'unfused-layer'), ('seg_head7', 'unfused-tail'),
            ('seg_head7', 'unfused-prologue'), ('seg_head7', 'sb-head'), ('seg_prologue', 'bf16x3'), ('seg_prologue', 'unfused-tail'),
            ('seg_ddpm', 'bf16x3'), ('seg_ddpm', 'f32'), ('seg_ddpm', 'unfused-prologue'),
            ('depth_chain', 'bf16x3'), ('depth_chain', 'f32'), ('depth_chain', 'unfused-tail'), ('depth_chain', 'unfused-prologue'),
            ('depth_lt', 'bf16x3'), ('depth_r2', 'bf16x3'), ('depth_r2', 'unfused-layer'), ('depth_L1', 'bf16x3'),
            ('depth_bins', 'bf16x3'), ('depth_bins', 'unfused-prologue'), ('depth_one_row', 'bf16x3'), ('depth_one_pixel', 'bf16x3'),
            ('bev_chain', 'bf16x3'), ('bev_chain', 'unfused-tail'), ('bev_chain', 'f32'), ('bev_separate', 'bf16x3'), ('bev_separate', 'f32'),
            ('x0_hints_seg', 'bf16x3'), ('x0_hints_seg', 'sb-head'), ('x0_hints_depth', 'bf16x3'), ('x0_hints_depth', 'unfused-tail'),
            ('prior_start_seg', 'bf16x3'), ('prior_start_seg', 'gather-refill'), ('prior_start_depth', 'bf16x3'),
            ('prior_start_bev', 'bf16x3'), ('prior_start_bev', 'unfused-tail'),
            ('class_prior', 'bf16x3'), ('class_prior', 'f32'), ('score_prior', 'bf16x3'), ('score_prior', 'unfused-tail'),
            ('score_and_class_prior', 'bf16x3'), ('ddpm_chain', 'chain'), ('ddpm_chain', 'chain-unfused-tail'),
            ('step_record_seeded_seg', 'seg_fused'), ('step_record_seeded_depth', 'depth_chain_1x37'),
            ('all_flags_seg', 'bf16x3'), ('all_flags_depth', 'bf16x3')]


def pairs():
    """[(target id, route id)] in a fixed order"""
    return [(tid, vid) for tid, t in TARGETS.items() for vid in t.routes]


def history_items():
    """[(target id, route id, polluter, fill)]: every polluter on the NaN-filled workspace; the polluters that move the geometry on a
    zero-filled one as well (see test_history_independence) - a polluter at the target's own geometry writes the rows the target
    call rewrites, and what it leaves elsewhere is loud on NaNs"""
    return [(tid, vid, p, f) for tid, vid in pairs() for p in TARGETS[tid].polluters(vid)
            for f in HISTORY_FILLS if f == 'nan' or p not in ('other_inputs', 'nan_inputs')]


SEQUENCE_TARGETS = [('all-seg', 'bf16x3'), ('all-depth', 'bf16x3'), ('cs-' + smallest_per_path()['depth_chain'], 'bf16x3'),
                    ('cs-' + smallest_per_path()['bev_chain'], 'bf16x3')]
GRAPH_TARGETS = [('cs-' + smallest_per_path()['seg_head7'], 'bf16x3'), ('dc-dc_15tok', 'chain'),
                 ('cs-' + smallest_per_path()['depth_chain'], 'bf16x3')]


def cfg_of(t, vid, geometry=None, lib=None):
    """the ``ddp_cfg`` of the route at ``geometry`` (default: the target's), made without a device: ``config_space_cases.make_cfg`` plus
    the flags the family adds, as ``DDPEngine.set_geometry`` moves it (the decoder grid follows the map except for bev)"""
    gemm, fl = t.routes[vid]
    fl = dict(fl)
    chain, refill = fl.pop('ddpm_chain', False), fl.pop('gather_guess_zero', False)
    cfg = S.make_cfg(t.c, gemm, **fl)
    k = dict(t.ekw, ddpm_chain=chain or t.ekw.get('ddpm_chain', False), gather_guess_zero=refill)
    for name, bit in (('record_x0', _lib.FLAG_RECORD_X0), ('gather_guess_zero', _lib.FLAG_GATHER_GUESS_ZERO),
                      ('record_steps', _lib.FLAG_STEP_RECORD), ('seeded_noise', _lib.FLAG_SEEDED_NOISE), ('ddpm_chain', _lib.FLAG_DDPM_CHAIN),
                      ('x0_hints', _lib.FLAG_X0_HINTS), ('prior_start', _lib.FLAG_PRIOR_START), ('class_prior', _lib.FLAG_CLASS_PRIOR),
                      ('score_prior', _lib.FLAG_SCORE_PRIOR)):
        if k.get(name):
            cfg.flags |= bit
    if geometry is not None:
        cfg.batch, cfg.h, cfg.w = geometry
        if t.c['task'] != 'bev':
            cfg.head_h, cfg.head_w = cfg.h, cfg.w
    return cfg


# ---- the FCN-head loop and the stand-alone entries ------------------------------------------------------------------------------
LOOPS = {'bn-cx64': ('next_rows_cases', N.LOOP['cx64']),                    # BatchNorm convs, 5 x 7, B = 2, a feature width of 64
         'gn-b2_ddpm_odd': ('fcn_gn_cases', G.LOOP['b2_ddpm_odd'])}         # GroupNorm(32) convs, 5 x 7, B = 2, ddpm, non-fused statistics
NECK_CASE, NECK_OTHER = 'flat_pyramid', 'mixed_low_ragged'                    # B = 1, 13 x 19 ... 2 x 2; the other geometry: B = 2, 9 x 7 ...
FCN_BN_CASE, FCN_BN_OTHER = '5x7_d1', 'three_maps_d3'                         # (N.FCN: BatchNorm convs)
FCN_GN_CASE, FCN_GN_OTHER = 'odd_3maps', 'wave_4x8'                           # (G.HEAD)
MSDA_SHAPE, MSDA_OTHER = (8, 16, 1), (13, 17, 2)                              # the smallest (h, w, r) of test_msda_forward_lds and its first
LINEAR_B3_SHAPE, LINEAR_B3_OTHER = (77, 152, 256), (300, 256, 256)            # (m, n, k): no multiple of a tile; test_linear's shapes
HEAD_FORWARD_CASE = 'seg_city_r2'                                             # test_head_forward_trace
ENTRIES = ['neck_fpn', 'neck_msm', 'neck_fpn_msm', 'fcn_head_bn', 'fcn_head_gn', 'msda_lds_wild', 'msda_lds_wild_guess', 'msda_lds_ring',
           'msda_lds_ring_guess', 'head_forward', 'linear_b3']


def msda_inputs(h, w, r, table):
    """value (r, n, 256), samp (r n, 96), offsets - the tables of tests/test_hip_parity.py::test_msda_forward_lds, and its reference"""
    import math
    from oracle import ddp_oracle as O
    n = h * w
    g = torch.Generator().manual_seed(h * 100 + w + (7 if table == 'ring' else 0))
    value = torch.randn(r, n, 8, 32, generator=g)
    if table == 'wild':
        off = torch.randn(r, n, 8, 4, 2, generator=g) * 3.0
        off[:, ::7] = torch.round(off[:, ::7])
        off[:, 3::11] *= 20.0
    else:
        th = torch.arange(8, dtype=torch.float32) * (2.0 * math.pi / 8)
        grid = torch.stack([th.cos(), th.sin()], -1)
        grid = grid / grid.abs().max(-1, keepdim=True).values
        ring = grid[:, None, :] * (torch.arange(4, dtype=torch.float32) + 1)[None, :, None]
        off = ring[None, None] + 0.3 * torch.randn(r, n, 8, 4, 2, generator=g)
    aw = torch.randn(r, n, 8, 4, generator=g).softmax(-1)
    jj = torch.arange(w, dtype=torch.float32).repeat(h)
    ii = torch.arange(h, dtype=torch.float32).repeat_interleave(w)
    px = jj[None, :, None, None] + off[..., 0]
    py = ii[None, :, None, None] + off[..., 1]
    ref = O.msda_core_taps(value, h, w, px, py, aw)
    samp = torch.cat([torch.stack((px, py), -1).reshape(r * n, 64), aw.reshape(r * n, 32)], 1).contiguous()
    return value.reshape(r, n, 256), samp, off.mean(dim=(0, 1, 3)), ref


def linear_b3_inputs(m, n, k):
    """a, w, bias and the fp64 product (tests/test_hip_parity.py::test_linear's operands)"""
    g = torch.Generator().manual_seed(m * 7 + n)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g)
    return a, w, b, torch.nn.functional.linear(a.double(), w.double(), b.double())


def query(lib, cfg):
    n = C.c_size_t(0)
    rc = lib.ddp_query_workspace(C.byref(cfg), C.byref(n))
    return rc, n.value
