"""CPU side of DDP_FLAG_PRIOR_START and ``t_start`` (tests/test_prior_start_gpu.py runs the cases on an MI355X): the schedule with
t_start = 1 is today's schedule bit for bit, the expectation loop of tests/prior_start_cases.py reduces to the oracle's four samplers
(bit for bit) when it starts from the noise at t = 1, is well conditioned and depends on the prior on every case; the flag's value,
the unchanged ABI, the workspace formulas, the unchanged flag-clear sizes, every refusal with its message, the host surface and the
resources of the new kernels.  No GPU compute is invoked."""
import ctypes as C
import inspect
import json
import os
import re
import shutil
import subprocess

import pytest
import torch

import config_space_cases as S
import prior_start_cases as P
from ddp_amd import _lib, schedule
from support import refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
FLAG_VARIANTS = [{}, dict(fused_tail=False), dict(nchw_head=False), dict(fused_layer=False), dict(fused_prologue=False)]


# ---- schedule -----------------------------------------------------------------------------------------------------------------------
def _old_pairs(timesteps, time_difference=1, sample_range0=0.0):
    """get_sampling_timesteps as it stood before t_start (ddp.py:204-213)"""
    times = []
    for step in range(timesteps):
        t_now = 1 - (step / timesteps) * (1 - sample_range0)
        t_next = max(1 - (step + 1 + time_difference) / timesteps * (1 - sample_range0), sample_range0)
        times.append((t_now, t_next))
    return times


def test_t_start_one_is_the_schedule_bit_for_bit():
    ks = list(range(1, 21)) + [31, 32, 50, 63, 64]
    for K in ks:
        for td in (0, 1, 2):
            for sr0 in (0.0, 0.001, 0.25, 0.5):
                want = _old_pairs(K, td, sr0)
                assert schedule.get_sampling_timesteps(K, td, sr0) == want
                assert schedule.get_sampling_timesteps(K, td, sr0, t_start=1.0) == want
                assert schedule.get_sampling_timesteps(K, td, sr0, 1) == want
    for task, sampler in (('seg', 'ddim'), ('seg', 'ddpm'), ('depth', 'ddim'), ('bev', 'ddim')):
        for ns in ('cosine', 'linear'):
            for K in (1, 2, 3, 7, 20, 64):
                for td in (0, 1, 2):
                    for sr0 in (0.0, 0.001, 0.3):
                        a = schedule.step_records(task, K, td, sr0, ns, sampler)
                        b = schedule.step_records(task, K, td, sr0, ns, sampler, t_start=1.0)
                        assert a == b and len(a) == K, (task, sampler, ns, K, td, sr0)


def test_t_start_divides_the_shorter_span():
    pairs = schedule.get_sampling_timesteps(3, 1, 0.0, t_start=0.6)
    assert pairs[0][0] == 0.6 and pairs[-1][1] == 0.0 and all(a > b for a, b in pairs)
    assert [round(a, 12) for a, _ in pairs] == [0.6, 0.4, 0.2]
    pairs = schedule.get_sampling_timesteps(2, 0, 0.1, t_start=0.5)
    assert pairs[0] == (0.5, 0.5 - 1 / 2 * (0.5 - 0.1)) and pairs[1][1] == 0.1
    r = schedule.step_records('seg', 2, 1, 0.0, 'cosine', 'ddim', t_start=0.25)[0]
    t = torch.tensor([0.25])
    al, si = schedule.log_snr_to_alpha_sigma(schedule.alpha_cosine_log_snr(t))
    assert r['alpha'] == float(al) and r['sigma'] == float(si)
    r = schedule.step_records('depth', 2, 1, 0.0, 'cosine', 'ddim', t_start=0.25)[0]
    g = schedule.gamma(t)
    assert r['time_in'] == 0.25 and r['alpha'] == float(g.sqrt()) and r['sigma'] == float(1 / (1 - g).sqrt())


@pytest.mark.parametrize('bad', [0.0, -0.1, 1.0000001, 2, float('nan'), float('inf')])
def test_t_start_bounds(bad):
    with pytest.raises(ValueError, match='t_start'):
        schedule.get_sampling_timesteps(3, 1, 0.0, t_start=bad)
    with pytest.raises(ValueError, match='t_start'):
        schedule.step_records('seg', 3, 1, 0.0, 'cosine', 'ddim', t_start=bad)


def test_t_start_must_lie_above_sample_range0():
    for t in (0.3, 0.2999):
        with pytest.raises(ValueError, match='t_start'):
            schedule.get_sampling_timesteps(3, 1, 0.3, t_start=t)
    assert len(schedule.get_sampling_timesteps(3, 1, 0.3, t_start=0.31)) == 3
    # depth and bev run on [0, t_start] whatever sample_range0 says (as step_records always did)
    assert len(schedule.step_records('depth', 3, 1, 0.5, 'cosine', 'ddim', t_start=0.2)) == 3


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def test_flag_value_abi_and_bars():
    assert _lib.FLAG_PRIOR_START == 65536 and _lib.ABI_VERSION == 7 and len(_lib.EXPORTS) == 36
    assert P.REL == 2e-4 and P.COND == 1e-5 and P.WITNESS == 2e-3
    header = open(os.path.join(ROOT, 'include', 'ddp_mi355x.h')).read()
    assert re.search(r'DDP_FLAG_PRIOR_START\s*=\s*65536\b', header) and '#define DDP_ABI_VERSION 7' in header
    assert not re.search(r'=\s*8192\b', header) and not re.search(r'=\s*32768\b', header)
    lib = _lib.load()
    assert lib.ddp_abi_version() == 7
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in out.splitlines() if ' T ' in l and 'ddp_' in l)
    assert syms == sorted(_lib.EXPORTS)
    assert C.sizeof(_lib.DdpCfg) == 136 and C.sizeof(_lib.DdpStep) == 32       # no struct grew
    from ddp_amd import build
    assert 'ddp_prior_start.hip' in build.SOURCES


def test_case_shapes():
    cs = P.CASES.values()
    assert {c['Kc'] for c in cs if c['task'] == 'seg'} == {1, 19, 150, 255, 256}
    assert P.T_STARTS == (1.0, 0.6, 0.25) and {c['t_start'] for c in cs} == {0.6, 0.25} and {c['K'] for c in cs} == {1, 2, 3}
    for c in cs:
        n = c['h'] * c['w']
        assert c['B'] in (2, 3) and c['L'] == 2
        assert c['task'] == 'bev' or (n % 4 != 0 and (c['B'] * c['r'] * n) % 32 != 0)
    assert [n for n, c in P.CASES.items() if not c['witness']] == ['seg_kc1_1x37']
    assert {(c['h'], c['w']) for c in cs if c['task'] == 'seg'} == {(7, 13), (9, 14), (5, 10), (1, 37), (1, 1), (3, 11)}
    assert {(c['h'], c['w']) for c in cs if c['task'] == 'depth'} == {(9, 14), (5, 10), (1, 37), (1, 1)}
    assert [c['sampler'] for c in cs if c['task'] == 'seg'].count('ddpm') == 1
    for n in ('bev_kc8_r1', 'bev_kc9_r2'):        # the geometry of the configuration sweep's cases
        for k in ('Kc', 'r', 'h', 'w', 'grid', 'threshold'):
            assert P.CASES[n][k] == S.CASES[n][k]


@pytest.mark.parametrize('name', sorted(P.CASES))
def test_prior_maps_hold_what_the_tests_need(name):
    c = P.CASES[name]
    B, N = c['B'], c['h'] * c['w']
    p0, p1 = P.prior(c, 0), P.prior(c, 1)
    assert p0.dtype == P.PRIOR_DTYPE[c['task']] and tuple(p0.shape) == (B, c['h'], c['w']) and not torch.equal(p0, p1)
    assert p0.numpy().tobytes() == P.prior(c, 0).numpy().tobytes()            # seeded (bytes: a depth map holds NaN)
    sd = P.state_dict(c)
    x0 = [P.x0_of_prior(c, sd, p0[b]).reshape(-1, N) for b in range(B)]
    for b in range(B - 1):                                                    # the map changes across the image border
        assert not torch.equal(x0[b][:, N - 1], x0[b + 1][:, 0]), (name, b)
    flat = p0.view(-1)
    if c['task'] == 'seg':
        flat = flat.long()
        ign = flat[flat >= c['Kc']]
        if c['Kc'] < 256:
            assert len(ign) and (c['Kc'] >= 254 or N == 1 or len(set(ign.tolist())) > 1)        # several ignore encodings
        else:
            assert len(ign) == 0 and int(flat.max()) > 250
        assert bool((flat < c['Kc']).any())
    elif c['task'] == 'depth':
        assert torch.isnan(flat).any()
        if N > 1:
            assert torch.isinf(flat).any() and (flat < 0).any() and (flat == 0).any()
            assert ((flat > 0) & (flat < c['min_depth'])).any() and (torch.isfinite(flat) & (flat > c['max_depth'])).any()
    else:
        word = flat.long() & 0xFFFFFFFF
        assert bool((word >> c['Kc']).bool().any()) and bool((word & ((1 << c['Kc']) - 1)).bool().any())      # bits >= num_classes too
        # ... and they are ignored
        clean = (word & ((1 << c['Kc']) - 1)).to(torch.int32).view_as(p0)
        assert torch.equal(P.x0_of_prior(c, sd, clean[0]), P.x0_of_prior(c, sd, p0[0]))


def test_x0_of_prior_is_the_reference_arithmetic():
    """seg: embedding row of the class, the last row for every ignore value (ddp.py:151); depth: the clamped normalisation, 0 for what
    is no depth; bev: the mean over the per-class rows"""
    c = P.CASES['seg_kc19_7x13']
    sd = P.state_dict(c)
    E = sd['embedding_table.weight']
    assert E.shape[0] == c['Kc'] + 1
    p = torch.tensor([[0, 5, 18, 19, 200, 255]], dtype=torch.uint8)
    x0 = P.x0_of_prior(c, sd, p)[0, :, 0]                                      # (256, 6)
    rows = [0, 5, 18, 19, 19, 19]
    for j, rw in enumerate(rows):
        assert torch.equal(x0[:, j], (torch.sigmoid(E[rw]) * 2 - 1) * c['bit_scale'])
    d = P.CASES['depth_9x14']
    lo, hi, bit = d['min_depth'], d['max_depth'], d['bit_scale']
    p = torch.tensor([[40.0, lo * 0.5, hi * 1.5, 0.0, -3.0, float('nan'), float('inf'), float('-inf')]])
    x0 = P.x0_of_prior(d, None, p)[0, 0, 0]
    assert x0[0] == ((torch.tensor(40.0) - lo) / (hi - lo) * 2 - 1) * bit and -bit <= x0[1] < -0.99 * bit and x0[2] == bit
    assert bool((x0[3:] == 0).all())
    b = P.CASES['bev_kc8_r1']
    sdb = P.state_dict(b)
    Eb = sdb['embedding_table.weight']
    p = torch.tensor([[0b101, 0]], dtype=torch.int32)
    x0 = P.x0_of_prior(b, sdb, p)[0, :, 0]
    rows = torch.stack([Eb[1], Eb[0], Eb[3]] + [Eb[0]] * 5).mean(0)
    assert torch.allclose(x0[:, 0], (torch.sigmoid(rows) * 2 - 1) * b['bit_scale'], rtol=0, atol=1e-8)
    assert torch.allclose(x0[:, 1], (torch.sigmoid(Eb[0]) * 2 - 1) * b['bit_scale'], rtol=0, atol=1e-8)


@pytest.mark.parametrize('name', sorted(P.CASES))
def test_noise_start_at_one_is_the_oracles_sampler_bit_for_bit(name):
    """the expectation loop from (noise, 1.0) == O.ddim_sample_seg / O.ddpm_sample_seg / O.sample_depth (binned: the sampler of
    tests/depth_bins_util.py) / O.ddim_sample_bev, torch.equal"""
    c = P.CASES[name]
    out, rec = P.expected(c, 'noise', t_start=1.0)
    sd = P.state_dict(c)
    x, noise, sn = S.inputs(c)
    ref = torch.cat([S.oracle_image(c, sd, x, noise, sn, b) for b in range(c['B'])], 0)
    assert out.dtype == torch.float32 and out.shape == ref.shape and torch.equal(out, ref)
    if c['task'] == 'seg':
        assert rec.shape == (c['K'], c['B'], c['r'], c['h'], c['w'])


@pytest.mark.parametrize('which', [0, 1, 'noise'])
@pytest.mark.parametrize('name', sorted(P.CASES))
def test_expectation_is_well_conditioned(name, which):
    """fp32 loop vs its own fp64 evaluation < COND = REL / 20, and - seg - the decisions agree at every step: the condition under which
    REL applies to the free-running GPU comparison unchanged.  No case is excused."""
    c = P.CASES[name]
    (o32, r32), (o64, r64) = P.expected(c, which, torch.float32), P.expected(c, which, torch.float64)
    err = P.max_rel(o32, o64)
    print(f'{name}/{which}: fp32 vs fp64 max-rel {err:.2e} (cap {P.COND:.0e})')
    assert o64.dtype == torch.float64 and torch.isfinite(o64).all() and err < P.COND
    if c['task'] == 'seg':
        assert torch.equal(r32, r64)


@pytest.mark.parametrize('name', sorted(P.CASES))
def test_the_prior_has_an_effect(name):
    """witness: prior start and noise start at the same t_start differ by more than 10 * REL - a GPU result within REL of one cannot
    be the other - and two different priors give different outputs.  (One class: one score channel, nothing to change.)"""
    c = P.CASES[name]
    a, b, n = P.expected(c, 0)[0], P.expected(c, 1)[0], P.expected(c, 'noise')[0]
    d_noise, d_prior = P.max_rel(a, n), P.max_rel(a, b)
    print(f'{name}: prior vs noise start {d_noise:.2e}, prior 0 vs prior 1 {d_prior:.2e}')
    if c['witness']:
        assert d_noise > P.WITNESS and d_prior > 0
    else:
        assert c['Kc'] == 1


# ---- the C surface ------------------------------------------------------------------------------------------------------------------
def _with(cfg, flags):
    n = _lib.DdpCfg.from_buffer_copy(cfg)
    n.flags |= flags
    return n


@pytest.mark.parametrize('name', sorted(P.CASES))
def test_workspace_grows_by_the_documented_buffers_only(name):
    """ddp_query_workspace with the flag = the value without + round256(prior_bytes) + [no SEEDED_NOISE: round256(start_bytes)], under
    every other flag and both engines; ddp_query_const_workspace unchanged"""
    lib = _lib.load()
    c = P.CASES[name]
    pb, sb = P.prior_bytes(c)
    n = c['B'] * c['h'] * c['w']
    assert pb == n * (1 if c['task'] == 'seg' else 4) and sb == n * c['r'] * (1 if c['task'] == 'depth' else 256) * 4
    extras = [0, _lib.FLAG_STEP_RECORD, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD | _lib.FLAG_SEEDED_NOISE, _lib.FLAG_GATHER_GUESS_ZERO]
    if c['task'] != 'bev' and c['Kc'] < 256:
        extras += [_lib.FLAG_X0_HINTS, _lib.FLAG_X0_HINTS | _lib.FLAG_SEEDED_NOISE | _lib.FLAG_STEP_RECORD]
    if c['task'] == 'seg':
        extras += [_lib.FLAG_RECORD_X0, _lib.FLAG_FORCE_X0, _lib.FLAG_FORCE_X0 | _lib.FLAG_SEEDED_NOISE]
        if c['sampler'] == 'ddpm':
            extras += [_lib.FLAG_DDPM_CHAIN, _lib.FLAG_DDPM_CHAIN | _lib.FLAG_SEEDED_NOISE]
    for gemm in ('bf16x3', 'f32'):
        for fl in FLAG_VARIANTS:
            for extra in extras:
                base = _with(S.make_cfg(c, gemm, **fl), extra)
                want = P.round256(pb) + (0 if extra & _lib.FLAG_SEEDED_NOISE else P.round256(sb))
                rc0, n0, m0 = S.query(lib, base)
                rc1, n1, m1 = S.query(lib, _with(base, _lib.FLAG_PRIOR_START))
                assert rc0 == 0 and rc1 == 0, lib.ddp_last_error().decode()
                assert n1 == n0 + want and m1 == m0, (name, gemm, fl, extra)


def test_flag_clear_gives_the_parents_workspace_sizes():
    """tests/golden/step_record/parent_workspace_bytes.json (recorded from an earlier build) on every case of the configuration
    sweep it holds: flag clear - those numbers; flag set - that total plus the formulas, that model region"""
    lib = _lib.load()
    golden = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'step_record', 'parent_workspace_bytes.json')))
    seen = 0
    for name, c in S.CASES.items():
        pb, sb = P.prior_bytes(c)
        for gemm in ('bf16x3', 'f32'):
            if f'{name}/{gemm}' not in golden['sample']:
                continue
            tot, const = golden['sample'][f'{name}/{gemm}']
            assert list(S.query(lib, S.make_cfg(c, gemm))) == [0, tot, const], (name, gemm)
            assert list(S.query(lib, _with(S.make_cfg(c, gemm), _lib.FLAG_PRIOR_START))) == [0, tot + P.round256(pb) + P.round256(sb), const]
            seen += 1
    assert seen > 60


def test_host_side_places_are_the_headers_formulas():
    """ddp_amd.engine.prior_start_places - the one host-side derivation - against the header's sentences, on a struct made without a
    device: the prior map in front of the hint buffers / the seeded-noise buffer / the step record, the start map in front of it or,
    with DDP_FLAG_SEEDED_NOISE, the seeded-noise buffer itself"""
    from ddp_amd.engine import prior_start_places, step_record_sizes
    lib = _lib.load()
    for name in ('seg_kc19_7x13', 'depth_5x10_r2', 'bev_kc9_r2'):
        c = P.CASES[name]
        pb, sb = P.prior_bytes(c)
        for extra in (0, _lib.FLAG_STEP_RECORD, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_SEEDED_NOISE | _lib.FLAG_STEP_RECORD) + \
                ((_lib.FLAG_X0_HINTS, _lib.FLAG_X0_HINTS | _lib.FLAG_SEEDED_NOISE | _lib.FLAG_STEP_RECORD) if c['task'] != 'bev' else ()):
            cfg = _with(S.make_cfg(c), extra | _lib.FLAG_PRIOR_START)
            rc, total, _ = S.query(lib, cfg)
            assert rc == 0
            end = total
            if extra & _lib.FLAG_STEP_RECORD:
                rec, smap = step_record_sizes(cfg)
                end -= P.round256(rec) + P.round256(smap)
            noise_at = None
            if extra & _lib.FLAG_SEEDED_NOISE:
                end -= P.round256(sb)
                noise_at = end
            if extra & _lib.FLAG_X0_HINTS:
                e = 1 if c['task'] == 'seg' else 4
                nb = c['B'] * c['h'] * c['w'] * e
                end -= P.round256(nb) + P.round256(nb * c['r'])
            prior_at = end - P.round256(pb)
            start_at = noise_at if noise_at is not None else prior_at - P.round256(sb)
            assert prior_start_places(cfg, total) == (prior_at, pb, start_at, sb), (name, extra)
            # ... and the first of the new buffers begins where the trailing buffers of the flag-clear cfg begin: every other offset
            # is the one of the cfg without the flag
            rc0, total0, _ = S.query(lib, _with(S.make_cfg(c), extra))
            trailing = total - (prior_at + P.round256(pb))
            assert rc0 == 0 and min(prior_at, start_at) == total0 - trailing


def test_refusals_carry_their_message():
    lib = _lib.load()
    # bev with more than 32 classes: the flag's own message in front of the class limit's
    b = dict(P.CASES['bev_kc9_r2'], Kc=33)
    refused(lib, _with(S.make_cfg(b), _lib.FLAG_PRIOR_START), 'DDP_FLAG_PRIOR_START', '32')
    refused(lib, S.make_cfg(b), 'bev supports at most 32 classes')
    assert S.query(lib, _with(S.make_cfg(dict(b, Kc=32)), _lib.FLAG_PRIOR_START))[0] == 0
    # seg with 256 classes is accepted (every byte value is a class)
    assert S.query(lib, _with(S.make_cfg(P.CASES['seg_kc256_3x11']), _lib.FLAG_PRIOR_START))[0] == 0
    # the FCN loop: workspace query, prepare and sample
    import seeded_noise_util as U
    n = C.c_size_t(0)
    for case in ('fcn_ddim', 'fcn_ddpm'):
        for flags in (0, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD):
            cfg = U.fcn_cfg(U.FCN_CASES[case], flags)
            assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == 0, lib.ddp_last_error()
            cfg.flags |= _lib.FLAG_PRIOR_START
            assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == -1
            assert b'sample_fcn: DDP_FLAG_PRIOR_START' in lib.ddp_last_error(), lib.ddp_last_error()
            # ddp_sample_fcn / ddp_prepare_fcn validate before they touch a pointer
            assert lib.ddp_sample_fcn(C.byref(cfg), None, None, 1, 1, None, None, None, None, None, None, None) == -1
            assert b'sample_fcn: DDP_FLAG_PRIOR_START' in lib.ddp_last_error(), lib.ddp_last_error()
            assert lib.ddp_prepare_fcn(C.byref(cfg), None, None, 1, 1, None, None, None) == -1
            assert b'sample_fcn: DDP_FLAG_PRIOR_START' in lib.ddp_last_error(), lib.ddp_last_error()
    # bits 8192 and 32768 are still bits nobody defines
    for bit in (8192, 32768):
        for extra in (bit, bit | _lib.FLAG_PRIOR_START):
            refused(lib, _with(S.make_cfg(P.CASES['seg_kc19_7x13']), extra), 'unknown flags')
            refused(lib, _with(S.make_cfg(P.CASES['depth_9x14']), extra), 'unknown flags')


# ---- host layer ---------------------------------------------------------------------------------------------------------------------
def test_engine_surface():
    """constructor keywords and methods of the host layer (no device needed to read them)"""
    from ddp_amd.engine import DDPEngine, FcnSamplerEngine, SampleGraph
    sig = inspect.signature(DDPEngine.__init__).parameters
    assert sig['prior_start'].default is False and sig['t_start'].default == 1.0
    assert inspect.signature(FcnSamplerEngine.__init__).parameters['prior_start'].default is False
    for m in ('prior_view', 'set_prior', 'clear_prior', 'last_start'):
        assert callable(getattr(DDPEngine, m))
    assert inspect.signature(SampleGraph.replay).parameters['prior'].default is None
    with pytest.raises(ValueError, match='prior_start'):
        FcnSamplerEngine({}, None, h=4, w=4, prior_start=True)
    # with both flags the seeded-noise buffer is the start map: last_noise() says so
    eng = object.__new__(DDPEngine)
    eng.seeded, eng._sampled = True, True
    eng.cfg = _with(S.make_cfg(P.CASES['seg_kc19_7x13']), _lib.FLAG_SEEDED_NOISE | _lib.FLAG_PRIOR_START)
    with pytest.raises(_lib.DdpError, match=r'last_start\(\)'):
        eng.last_noise()
    eng.cfg = _with(S.make_cfg(P.CASES['seg_kc19_7x13']), _lib.FLAG_SEEDED_NOISE)
    with pytest.raises(_lib.DdpError, match='prior_start'):
        eng.prior_view()
    with pytest.raises(_lib.DdpError, match='prior_start'):
        eng.last_start()


def test_plugin_surface_without_a_device():
    """``prior=None, t_start=None`` are call-time arguments of the plugin classes, their constructors stay the reference's; aug_test and
    slide inference raise ValueError; nearest resampling by the rule of ``_hint_map``"""
    from ddp_amd import apis
    from ddp_amd.bev.ddp import DDP as BevDDP
    from ddp_amd.depther.ddp import DDP as DepthDDP
    from ddp_amd.segmentors.ddp import DDP as SegDDP
    for cls, methods in ((SegDDP, ('ddim_sample', 'ddpm_sample', 'simple_test', 'forward', 'aug_test', 'slide_inference')),
                         (DepthDDP, ('sample', 'simple_test', 'inference', 'aug_test')), (BevDDP, ('ddim_sample',))):
        for k in ('prior', 't_start', 'prior_start'):
            assert k not in inspect.signature(cls.__init__).parameters
        for m in methods:
            p = inspect.signature(getattr(cls, m)).parameters
            assert p['prior'].default is None and p['t_start'].default is None, (cls, m)
    p = inspect.signature(SegDDP._engine_for).parameters
    assert p['prior'].default is False and p['t_start'].default is None
    for cls in (SegDDP, DepthDDP):
        for kw in (dict(prior=torch.zeros(1, 2, 2), t_start=0.5), dict(t_start=0.5)):
            with pytest.raises(ValueError, match='prior'):
                cls.aug_test(object.__new__(cls), [None, None], [None, None], **kw)
    for kw in (dict(prior=torch.zeros(1, 2, 2), t_start=0.5), dict(t_start=0.5)):
        with pytest.raises(ValueError, match='prior'):
            SegDDP.slide_inference(object.__new__(SegDDP), None, None, False, **kw)
    with pytest.raises(ValueError, match='t_start'):                             # a prior without a time
        SegDDP._check_t_start(torch.zeros(1, 2, 2), None)
    # nearest resampling at a non-integer ratio: floats through F.interpolate, integers by the same index rule - bit words survive
    src = torch.zeros(2, 7, 9)
    src[:, 3, 4] = 50.0
    m = SegDDP._prior_map([src], 2, 3, 4, torch.float32)
    assert torch.equal(m, torch.nn.functional.interpolate(src[:, None], size=(3, 4), mode='nearest')[:, 0])
    g = torch.Generator().manual_seed(5)
    words = torch.randint(-2 ** 31, 2 ** 31 - 1, (2, 7, 9), generator=g).to(torch.int32)
    m = SegDDP._prior_map(words, 2, 3, 4, torch.int32)
    ys = torch.floor(torch.arange(3, dtype=torch.float32) * (7 / 3)).long()
    xs = torch.floor(torch.arange(4, dtype=torch.float32) * (9 / 4)).long()
    assert m.dtype == torch.int32 and torch.equal(m, words[:, ys[:, None], xs[None, :]])
    cls8 = torch.randint(0, 256, (2, 7, 9), generator=g).to(torch.uint8)
    m8 = SegDDP._prior_map(cls8, 2, 3, 4, torch.uint8)
    assert m8.dtype == torch.uint8
    assert torch.equal(m8, torch.nn.functional.interpolate(cls8[:, None].float(), size=(3, 4), mode='nearest')[:, 0].to(torch.uint8))
    for bad in (torch.zeros(3, 7, 9), torch.zeros(7, 9), [src, src], 'x'):
        with pytest.raises(ValueError, match='prior'):
            SegDDP._prior_map(bad, 2, 3, 4, torch.uint8)
    # the harness hands a ``prior`` entry of the batch through, on the model's device
    seen = {}

    class _M(torch.nn.Module):
        def forward(self, **kw):
            seen.update(kw)
            return []
    apis._run_batch(_M(), dict(img=[torch.zeros(1, 3, 4, 4)], img_metas=[None], prior=[torch.zeros(1, 4, 4)], t_start=0.5), torch.device('cpu'))
    assert torch.is_tensor(seen['prior'][0]) and seen['t_start'] == 0.5 and seen['return_loss'] is False


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_prior_start_kernel_resources(tmp_path):
    """k_prior_start_tab (seg, bev) / k_prior_start_depth for gfx950: no scratch; LDS = the slab of 32 channels x (rows) with the one
    pad float per row and nothing else - seg 257 rows (256 classes + the ignore row), bev 33, depth none.  Registers as found when the
    kernels were written: seg 97, bev 61, depth 30 (asserted with a little room: at most 128, which keeps 4 waves per SIMD)."""
    out = tmp_path / 'prior_start.s'
    src = os.path.join(ROOT, 'ddp_amd', 'csrc', 'ddp_prior_start.hip')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-x', 'hip', src,
                    '--cuda-device-only', '-S', '-o', str(out)], check=True, capture_output=True, timeout=600)
    found = re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', out.read_text(), re.S)
    assert len(found) == 3
    lds_cap = {'k_prior_start_tabILb0ELi257': 257 * 33 * 4, 'k_prior_start_tabILb1ELi33': 33 * 33 * 4, 'k_prior_start_depth': 0}
    seen = set()
    for name, body in found:
        key = [k for k in lds_cap if k in name]
        assert len(key) == 1, name
        seen.add(key[0])
        vgpr = int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1))
        lds = int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1))
        print(f'{name}: {vgpr} registers, {lds} B LDS')
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert lds <= lds_cap[key[0]], name
        assert vgpr <= 128, name
    assert seen == set(lds_cap)
