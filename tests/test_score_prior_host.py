"""CPU side of DDP_FLAG_SCORE_PRIOR (tests/test_score_prior_gpu.py runs the cases on an MI355X): the seeds of
tests/score_prior_cases.py are the first that meet the margin rule; the expectation - the oracle's sampler through its ``head=`` hook -
reduces to the oracle's own result with a zero map, to the class prior family's expectation with a constant map and is well
conditioned; the flag's value, the unchanged ABI, the workspace formulas, the table of caller regions, every refusal with its message,
the compiled resources of the kernels that changed and the device-free host surface.  No GPU compute is invoked."""
import ctypes as C
import inspect
import itertools
import os
import re
import shutil
import subprocess

import pytest
import torch

import class_prior_cases as PC
import config_space_cases as S
import score_prior_cases as P
from ddp_amd import _lib
from support import refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
CASE_KINDS = [(n, k) for n in P.CASES for k in P.SEEDED_KINDS]
SEED_KINDS = CASE_KINDS + [(n, 'both') for n in P.BOTH]
TAIL = (_lib.FLAG_CLASS_PRIOR, _lib.FLAG_PRIOR_START, _lib.FLAG_X0_HINTS, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD)


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def test_flag_value_abi_and_header():
    assert _lib.FLAG_SCORE_PRIOR == 1048576 == 1 << 20 and _lib.ABI_VERSION == 7 and len(_lib.EXPORTS) == 36
    assert P.REL == 2e-4 and P.COND == 1e-5 and P.MARGIN == 1e-3 == 5 * P.REL and P.CLAMP == 1e30
    header = open(os.path.join(ROOT, 'include', 'ddp_mi355x.h')).read()
    assert re.search(r'DDP_FLAG_SCORE_PRIOR\s*=\s*1048576\b', header) and '#define DDP_ABI_VERSION 7' in header
    for undefined in (8192, 32768, 262144, 524288):
        assert not re.search(r'=\s*%d\b' % undefined, header), undefined
    assert 'Bits 8192, 32768, 262144 and 524288 stay undefined' in re.sub(r'\s+', ' ', header)      # the header says which bits
    assert '/* score prior (DDP_FLAG_SCORE_PRIOR' in header
    assert '0. DDP_FLAG_SCORE_PRIOR: round256(rows_bytes), then round256(map_bytes)' in header
    assert header.index('0. DDP_FLAG_SCORE_PRIOR') < header.index('1. DDP_FLAG_CLASS_PRIOR')
    for words in ('map_bytes  = batch * num_classes * h * w * 4', 'rows_bytes = batch * h * w * KP * 4', 'KP = 64 * ceil(num_classes / 64)',
                  'one k_score_prior_rows per call', 'both priors add', 'never initialises the map'):
        assert words in header, words
    lib = _lib.load()
    assert lib.ddp_abi_version() == 7
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in out.splitlines() if ' T ' in l and 'ddp_' in l)
    assert syms == sorted(_lib.EXPORTS) and len(syms) == 36
    assert C.sizeof(_lib.DdpCfg) == 136 and C.sizeof(_lib.DdpStep) == 32       # no struct grew
    from ddp_amd import build
    assert 'ddp_score_prior.hip' in build.SOURCES


def test_case_shapes():
    cs = P.CASES
    geo = {n: (c['h'], c['w'], c['Kc'], c['B'], c['r']) for n, c in cs.items()}
    assert geo == {'kc19_7x13_b3': (7, 13, 19, 3, 1), 'kc19_8x12_b2': (8, 12, 19, 2, 1), 'kc255_5x10_r2': (5, 10, 255, 2, 2),
                   'kc256_3x11': (3, 11, 256, 2, 1), 'kc150_9x14_noacc': (9, 14, 150, 2, 1), 'kc64_4x9': (4, 9, 64, 2, 1),
                   'kc65_4x9': (4, 9, 65, 2, 1), 'kc1_1x37': (1, 37, 1, 2, 1), 'kc19_37x1': (37, 1, 19, 2, 1),
                   'kc19_1x1_b3': (1, 1, 19, 3, 1), 'ddpm_7x13': (7, 13, 19, 2, 1)}
    assert [n for n, c in cs.items() if not c['accumulation']] == ['kc150_9x14_noacc']
    assert [n for n, c in cs.items() if c['sampler'] == 'ddpm'] == ['ddpm_7x13']
    assert [n for n, c in cs.items() if not c['witness']] == ['kc1_1x37']
    assert P.BOTH == ['kc19_7x13_b3', 'kc255_5x10_r2', 'ddpm_7x13']
    for i, c in enumerate(cs.values()):
        assert c['K'] in (1, 2, 3) and c['L'] == 2 and c['task'] == 'seg' and c['base'] == 3000 + 100 * i
    assert {c['K'] for c in cs.values()} == {1, 2, 3}
    # image borders inside a 32-token tile / on tile borders; the chunk edge of KP
    assert (7 * 13) % 32 != 0 and (8 * 12) % 32 == 0 and 3 * 1 < 32
    assert P.kp(cs['kc64_4x9']) == 64 and P.kp(cs['kc65_4x9']) == 128 and P.kp(cs['kc1_1x37']) == 64 and P.kp(cs['kc256_3x11']) == 256
    assert P.kp(cs['kc150_9x14_noacc']) == 192 and P.KINDS == ('soft', 'excl', 'odd', 'const', 'zero')


@pytest.mark.parametrize('name', list(P.CASES))
def test_maps_hold_what_the_tests_need(name):
    c = P.CASES[name]
    shape = (c['B'], c['Kc'], c['h'], c['w'])
    for kind in P.KINDS:
        m = P.prior_map(c, kind)
        assert m.dtype == torch.float32 and tuple(m.shape) == shape and m.is_contiguous()
        assert m.numpy().tobytes() == P.prior_map(c, kind).numpy().tobytes()                # seeded
    soft = P.prior_map(c, 'soft')
    assert set(soft.unique().tolist()) <= {-3.0, 0.0, 3.0}
    assert abs(float((soft != 0).float().mean()) - 1 / 3) < (0.2 if soft.numel() < 200 else 0.06)
    flat = soft.reshape(c['B'], c['Kc'], -1)
    if c['Kc'] >= 19 and flat.shape[2] > 1:                                                 # another row at every pixel
        assert bool((flat[:, :, 1:] != flat[:, :, :-1]).any(1).all())
    excl = P.prior_map(c, 'excl')
    base = P.expected(c, 'none', seed_of='excl')['out'].argmax(1)
    assert bool((torch.isinf(excl) & (excl < 0)).sum(1).eq(1).all())                        # one class per pixel ...
    assert torch.equal(excl.argmin(1), base) and bool((excl.nan_to_num(neginf=0.0) == 0).all())   # ... the one decided without a prior
    odd = P.prior_map(c, 'odd')
    assert bool(torch.isnan(odd).any()) and bool((odd == float('inf')).any()) and bool((odd == float('-inf')).any())
    fin = torch.isfinite(odd)
    assert torch.equal(odd[fin], soft[fin])
    cl = P.clamp(odd)
    big = float(torch.tensor(1e30, dtype=torch.float32))                                    # (fl32(1e30) lies a little above 1e30)
    assert bool(torch.isfinite(cl).all()) and float(cl.max()) == big and float(cl.min()) == -big and bool((cl[torch.isnan(odd)] == 0).all())
    const = P.prior_map(c, 'const')
    assert torch.equal(const, P.const_rows(c)[:, :, None, None].expand(shape)) and (c['Kc'] == 1 or bool((P.const_rows(c) != 0).any()))
    assert not bool(P.prior_map(c, 'zero').any())
    # the rows buffer the kernel must write: token-major, normalised, zero padded
    rows = P.rows_of(odd, c)
    n = c['h'] * c['w']
    assert tuple(rows.shape) == (c['B'] * n, P.kp(c)) and not bool(rows[:, c['Kc']:].any())
    for b, k, i in ((0, 0, 0), (c['B'] - 1, c['Kc'] - 1, n - 1), (c['B'] - 1, c['Kc'] // 2, n // 2)):
        assert float(rows[b * n + i, k]) == float(cl[b, k].reshape(-1)[i])


@pytest.mark.parametrize('name,kind', SEED_KINDS)
def test_seeds_are_the_first_that_meet_the_margin_rule(name, kind):
    """the rule of the case file - fp64 top-2 margin >= MARGIN at every pixel and step (and the witness for 'excl') - searched on the
    CPU from the case's base; here the last SEARCH_WINDOW steps of that search: every seed in front of the chosen one fails, it passes"""
    c = P.CASES[name]
    seed = c['seeds'][kind]
    assert seed >= c['base'] and P.SEARCH_WINDOW == 10
    assert P.first_seed(c, kind, start=max(c['base'], seed - P.SEARCH_WINDOW)) == seed


@pytest.mark.parametrize('name,kind', CASE_KINDS)
def test_expectation_is_well_conditioned_decides_with_margin_and_has_its_witness(name, kind):
    """fp32 vs fp64 < 1e-5 and the same decisions at every step; in fp64 the top-2 margin of every pixel at every step is >= 1e-3 of the
    step's largest score: no pixel is excused on the GPU.  'excl': every pixel's final decision changes and the excluded class is
    never decided there, at any step, by any replica; its accumulated probability is exactly 0 / its returned score finite."""
    c = P.CASES[name]
    e32, e64 = P.expected(c, kind), P.expected(c, kind, torch.float64)
    err = P.max_rel(e32['out'], e64['out']) if kind == 'soft' else _rel_live(e32['out'], e64['out'], P.prior_map(c, kind))
    print(f'SCORE-PRIOR {name}/{kind} seed {c["seeds"][kind]}: fp32 vs fp64 {err:.2e} (cap 1e-05), fp64 top-2 margin '
          f'{e64["margin"]:.2e} (floor {P.MARGIN:.0e})')
    assert e64['out'].dtype == torch.float64 and torch.isfinite(e64['out']).all() and torch.isfinite(e32['out']).all()
    assert err < 1e-5 and torch.equal(e32['record'], e64['record'])
    assert e64['margin'] >= P.MARGIN and e32['margin'] >= P.MARGIN * 0.99
    assert tuple(e32['record'].shape) == (c['K'], c['B'], c['r'], c['h'], c['w'])
    base = P.expected(c, 'none', seed_of=kind)['out'].argmax(1)
    fin = e32['out'].argmax(1)
    if kind == 'soft':
        assert not c['witness'] or float((fin != base).float().mean()) >= 0.1               # the prior is felt
        return
    if not c['witness']:
        assert c['Kc'] == 1
        return
    assert P.excl_witness(c, base, e32) and P.excl_witness(c, base, e64)
    at = e32['out'].gather(1, base[:, None])
    if c['accumulation']:
        assert bool((at == 0).all())                                                        # softmax term exactly 0 at every step
    else:
        assert float(at.max()) <= -9e29


@pytest.mark.parametrize('name', P.BOTH)
def test_both_priors_expectation_decides_with_margin(name):
    """the soft map and the class-prior rows together (DDP_FLAG_CLASS_PRIOR + DDP_FLAG_SCORE_PRIOR), on the 'both' seed"""
    c = P.CASES[name]
    e32, e64 = P.expected(c, 'both'), P.expected(c, 'both', torch.float64)
    err = P.max_rel(e32['out'], e64['out'])
    print(f'SCORE-PRIOR {name}/both seed {c["seeds"]["both"]}: fp32 vs fp64 {err:.2e}, fp64 top-2 margin {e64["margin"]:.2e}')
    assert err < 1e-5 and torch.equal(e32['record'], e64['record']) and e64['margin'] >= P.MARGIN
    alone = P.expected(c, 'soft', seed_of='both')
    assert not torch.equal(alone['out'], e32['out'])                                        # the class rows are felt on top of the map


_rel_live = P.rel_live


@pytest.mark.parametrize('name', list(P.CASES))
def test_zero_map_is_the_oracles_sampler_bit_for_bit(name):
    """the expectation with the zero map == tests/config_space_cases.oracle_image (O.ddim_sample_seg / O.ddpm_sample_seg), torch.equal:
    fl32(score + 0) is the score, the hook changes nothing else"""
    c = P.seeded(P.CASES[name], 'zero')
    e = P.expected(c, 'zero')
    sd = S.state_dict(c)
    x, noise, sn = S.inputs(c)
    ref = torch.cat([S.oracle_image(c, sd, x, noise, sn, b) for b in range(c['B'])], 0)
    assert e['out'].dtype == torch.float32 and torch.equal(e['out'], ref)
    assert torch.equal(P.expected(c, 'none')['out'], ref)


@pytest.mark.parametrize('name', ['kc19_7x13_b3', 'kc150_9x14_noacc', 'kc255_5x10_r2', 'kc65_4x9', 'ddpm_7x13'])
def test_constant_map_is_the_class_priors_expectation(name):
    """a map constant over the pixels of each image against tests/class_prior_cases.expected with that row (the oracle on a state dict
    whose conv_seg.bias is fl32(bias + row)): the same decisions at every step and the same output.  The two expectations round
    differently - fl32(fl32(W q + bias) + p) here, fl32(W q + fl32(bias + p)) there - so on the CPU they agree to fp32 rounding
    (measured <= 1.3e-6 of the largest output, asserted below the project's conditioning cap 1e-5), not bit for bit; the LIBRARY gives
    the same bits for both flags on every route (tests/test_score_prior_gpu.py)."""
    c = P.seeded(P.CASES[name], 'const')
    e = P.expected(c, 'const')
    w = PC.expected(c, 'soft')
    err = P.max_rel(e['out'], w['out'])
    print(f'SCORE-PRIOR {name}/const vs the class prior expectation: {err:.2e}')
    assert torch.equal(e['record'], w['record']) and err < P.COND


# ---- the C surface ------------------------------------------------------------------------------------------------------------------
FLAG_VARIANTS = [dict(zip(('fused_layer', 'fused_prologue', 'fused_tail', 'nchw_head'), v)) for v in itertools.product((True, False), repeat=4)]


def _with(cfg, flags):
    n = _lib.DdpCfg.from_buffer_copy(cfg)
    n.flags |= flags
    return n


def _tail_sets(c):
    """every combination of the other five tail flags (and the two x0 instruments) that validate accepts for the case"""
    out = []
    for bits in itertools.product((0, 1), repeat=7):
        f = sum(b for b, on in zip(TAIL + (_lib.FLAG_RECORD_X0, _lib.FLAG_FORCE_X0), bits) if on)
        if f & _lib.FLAG_X0_HINTS and (c['Kc'] > 255 or f & _lib.FLAG_FORCE_X0):
            continue
        if f & _lib.FLAG_STEP_RECORD and f & _lib.FLAG_FORCE_X0:
            continue
        out.append(f)
    if c['sampler'] == 'ddpm':
        out += [f | _lib.FLAG_DDPM_CHAIN for f in out[:8]]
    return out


@pytest.mark.parametrize('name', list(P.CASES))
def test_workspace_grows_by_the_two_documented_buffers_only(name):
    """ddp_query_workspace with the flag = the value without + round256(rows_bytes) + round256(map_bytes), the two formulas written out
    here, under every combination of the other tail flags, on both engines and all route flag sets; ddp_query_const_workspace unchanged"""
    lib = _lib.load()
    c = dict(P.CASES[name], seed=1)
    n = c['B'] * c['h'] * c['w']
    map_bytes = c['B'] * c['Kc'] * c['h'] * c['w'] * 4
    rows_bytes = n * 64 * -(-c['Kc'] // 64) * 4
    assert (map_bytes, rows_bytes) == P.prior_bytes(c)
    grow = (map_bytes + 255) // 256 * 256 + (rows_bytes + 255) // 256 * 256
    seen = 0
    for gemm in ('bf16x3', 'f32'):
        for fl in FLAG_VARIANTS:
            for extra in _tail_sets(c):
                base = _with(S.make_cfg(c, gemm, **fl), extra)
                rc0, n0, m0 = S.query(lib, base)
                rc1, n1, m1 = S.query(lib, _with(base, _lib.FLAG_SCORE_PRIOR))
                assert rc0 == 0 and rc1 == 0, (extra, lib.ddp_last_error().decode())
                assert n1 == n0 + grow and m1 == m0, (name, gemm, fl, extra)
                seen += 1
    assert seen >= 2 * 16 * 48                     # (256 classes: no hints; every other case 72 or more flag sets)


def test_caller_regions_tile_the_end_of_the_workspace():
    """ddp_amd.engine.caller_regions with the flag: sprior_rows, sprior_map in front of cprior_rows, contiguous 256-aligned regions
    that end at ddp_query_workspace and begin where the workspace of the cfg without the six flags ends; score_prior_places is a
    lookup into the table and the header's place of the map"""
    from ddp_amd.engine import caller_regions, score_prior_places
    lib = _lib.load()
    order = ['sprior_rows', 'sprior_map', 'cprior_rows', 'cprior_table', 'prior_start', 'prior_map', 'hint_rows', 'hint_map', 'seed_noise',
             'step_rec', 'step_map']
    for name in ('kc19_7x13_b3', 'kc255_5x10_r2', 'kc65_4x9', 'kc19_1x1_b3', 'ddpm_7x13'):
        c = dict(P.CASES[name], seed=1)
        mb, rb = P.prior_bytes(c)
        for gemm in ('bf16x3', 'f32'):
            bare = S.query(lib, S.make_cfg(c, gemm))[1]
            for extra in _tail_sets(c):
                if extra & (_lib.FLAG_RECORD_X0 | _lib.FLAG_FORCE_X0 | _lib.FLAG_DDPM_CHAIN):
                    continue
                cfg = _with(S.make_cfg(c, gemm), extra | _lib.FLAG_SCORE_PRIOR)
                rc, total, _ = S.query(lib, cfg)
                assert rc == 0
                regions = caller_regions(cfg, total)
                names = list(regions)
                assert names[:2] == ['sprior_rows', 'sprior_map'] and names == [n for n in order if n in regions]
                assert ('cprior_rows' in regions) == bool(extra & _lib.FLAG_CLASS_PRIOR)
                at = bare
                for nm, (off, nbytes) in regions.items():
                    assert off == at and off % 256 == 0 and nbytes > 0, (name, extra, nm)
                    at = off + P.round256(nbytes)
                assert at == total
                assert regions['sprior_rows'][1] == rb and regions['sprior_map'][1] == mb
                assert score_prior_places(cfg, total) == regions['sprior_map'] + regions['sprior_rows']
                # every other region lies where it lies without the flag, moved by the group's size
                without = caller_regions(_with(S.make_cfg(c, gemm), extra), total - P.round256(rb) - P.round256(mb))
                assert {k: (o + P.round256(rb) + P.round256(mb), b) for k, (o, b) in without.items()} == \
                    {k: v for k, v in regions.items() if not k.startswith('sprior')}
    flagless = S.make_cfg(dict(P.CASES['kc19_7x13_b3'], seed=1))
    assert caller_regions(flagless, S.query(lib, flagless)[1]) == {}


def test_refusals_carry_their_message():
    import prior_start_cases as PS
    import seeded_noise_util as U
    lib = _lib.load()
    seg = dict(P.CASES['kc19_7x13_b3'], seed=1)
    for other in ('depth_9x14', 'depth_1x37_bins', 'bev_kc8_r1', 'bev_kc9_r2'):
        base = S.make_cfg(PS.CASES[other])
        assert S.query(lib, base)[0] == 0
        refused(lib, _with(base, _lib.FLAG_SCORE_PRIOR), 'DDP_FLAG_SCORE_PRIOR exists for the segmentation sampler only')
    n = C.c_size_t(0)
    for case in ('fcn_ddim', 'fcn_ddpm'):
        for flags in (0, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD):
            cfg = U.fcn_cfg(U.FCN_CASES[case], flags)
            assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == 0, lib.ddp_last_error()
            cfg.flags |= _lib.FLAG_SCORE_PRIOR
            assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == -1
            assert b'sample_fcn: DDP_FLAG_SCORE_PRIOR is built for ddp_sample only' in lib.ddp_last_error(), lib.ddp_last_error()
            # ddp_sample_fcn / ddp_prepare_fcn validate before they touch a pointer
            assert lib.ddp_sample_fcn(C.byref(cfg), None, None, 1, 1, None, None, None, None, None, None, None) == -1
            assert b'sample_fcn: DDP_FLAG_SCORE_PRIOR' in lib.ddp_last_error(), lib.ddp_last_error()
            assert lib.ddp_prepare_fcn(C.byref(cfg), None, None, 1, 1, None, None, None) == -1
            assert b'sample_fcn: DDP_FLAG_SCORE_PRIOR' in lib.ddp_last_error(), lib.ddp_last_error()
    # the bits nobody defines stay refused, with and without the new flag
    for bit in (8192, 32768, 262144, 1 << 19, 1 << 21, 1 << 30):
        for extra in (bit, bit | _lib.FLAG_SCORE_PRIOR):
            refused(lib, _with(S.make_cfg(seg), extra), 'unknown flags')
    # what combines: every other flag of ddp_sample, 256 classes included
    for name, c in P.CASES.items():
        c = dict(c, seed=1)
        for extra in _tail_sets(c):
            assert S.query(lib, _with(S.make_cfg(c), extra | _lib.FLAG_SCORE_PRIOR))[0] == 0, (name, extra, lib.ddp_last_error())


# ---- compiled resources -------------------------------------------------------------------------------------------------------------
def _compile(tmp, src_name):
    out = os.path.join(tmp, src_name + '.s')
    src = os.path.join(ROOT, 'ddp_amd', 'csrc', src_name)
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-x', 'hip', src,
                    '--cuda-device-only', '-S', '-o', out], check=True, capture_output=True, timeout=900)
    res = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', open(out).read(), re.S):
        body = m.group(2)
        res[m.group(1)] = tuple(int(re.search(r'\.amdhsa_%s (\d+)' % k, body).group(1))
                                for k in ('private_segment_fixed_size', 'next_free_vgpr', 'group_segment_fixed_size'))
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_rows_kernel_and_seg_update_resources(tmp_path):
    """k_score_prior_rows: no scratch, the (64, 68) float tile = 17408 B of LDS and 51 registers as measured (16 loads in flight per
    lane) - bounds: exactly 17408 B, <= 64 registers (the last count at which 8 waves per SIMD fit);
    k_seg_update stays one kernel without scratch or LDS in <= 64 registers; k_class_prior (it shares the normalisation) keeps its bounds.
    (The k_layer statements - no scratch, <= 512 registers, the flag-clear tails at exactly the parent's registers, 4 or 8 forced
    instantiations - are tests/test_class_prior_host.py's, which runs on these sources.)"""
    from concurrent.futures import ThreadPoolExecutor
    srcs = ['ddp_score_prior.hip', 'ddp_kernels.hip', 'ddp_class_prior.hip']
    with ThreadPoolExecutor(3) as ex:
        compiled = dict(zip(srcs, ex.map(lambda s: _compile(str(tmp_path), s), srcs)))
    ks = compiled['ddp_score_prior.hip']
    assert len(ks) == 1
    (name, (scratch, vgpr, lds)), = ks.items()
    print(f'k_score_prior_rows: {vgpr} registers, {lds} B LDS, {scratch} B scratch')
    assert 'k_score_prior_rows' in name and scratch == 0 and lds == 64 * 68 * 4 == 17408 and vgpr <= 64
    upd = {k: v for k, v in compiled['ddp_kernels.hip'].items() if 'k_seg_update' in k}
    assert len(upd) == 1
    (scratch, vgpr, lds), = upd.values()
    print(f'k_seg_update: {vgpr} registers')
    assert scratch == 0 and lds == 0 and vgpr <= 64
    (cname, (scratch, vgpr, lds)), = compiled['ddp_class_prior.hip'].items()
    assert 'k_class_prior' in cname and scratch == 0 and lds == 0 and vgpr <= 32
    # the layer kernel's new argument is appended behind cp_rn and adds no template parameter
    hdr = open(os.path.join(ROOT, 'ddp_amd', 'csrc', 'layer_bf16x3.h')).read()
    args = hdr[hdr.index('struct LayerArgs'):hdr.index('// vmcnt(12)')]
    assert args.index('int cp_rn;') < args.index('const float* sp_rows;') and args.rstrip().endswith('};')
    tmpl = re.search(r'template <([^>]*)>\s*__global__[^{]*k_layer\(LayerArgs la\)', hdr).group(1)
    assert tmpl.count(',') == 4 and 'bool FORCE' in tmpl                       # TAG, MODE, NCH, NT, FORCE: the parent's five


# ---- host layer ---------------------------------------------------------------------------------------------------------------------
def test_engine_surface():
    from ddp_amd import engine
    from ddp_amd.engine import DDPEngine, FcnSamplerEngine, SampleGraph, score_prior_places
    assert inspect.signature(DDPEngine.__init__).parameters['score_prior'].default is False
    assert inspect.signature(FcnSamplerEngine.__init__).parameters['score_prior'].default is False
    for m in ('score_prior_view', 'set_score_prior', 'clear_score_prior'):
        assert callable(getattr(DDPEngine, m))
    assert inspect.signature(SampleGraph.replay).parameters['score_prior'].default is None
    with pytest.raises(ValueError, match='score_prior is built for ddp_sample only'):
        FcnSamplerEngine({}, None, h=4, w=4, score_prior=True)
    assert callable(score_prior_places)
    every = S.make_cfg(dict(P.CASES['kc19_7x13_b3'], seed=1))
    every.flags |= _lib.FLAG_SCORE_PRIOR | _lib.FLAG_CLASS_PRIOR | _lib.FLAG_PRIOR_START | _lib.FLAG_X0_HINTS
    names = list(engine.caller_regions(every, 1 << 24))
    assert names.index('sprior_rows') < names.index('sprior_map') < names.index('cprior_rows')
    assert [row.region for row in engine.CALLER_INPUTS] == [n for n in names if n in ('sprior_map', 'cprior_table', 'prior_map', 'hint_map')]
    assert [row.name for row in engine.CALLER_INPUTS] == ['score_prior', 'class_prior', 'prior', 'hints']
    # ... and is, field for field, the literal rows the conditioning tests run on
    import conditioning_cases as CC
    tasks = {_lib.TASK_SEG: 'seg', _lib.TASK_DEPTH: 'depth', _lib.TASK_BEV: 'bev'}
    assert [(r.name, r.kwarg, r.flag, r.flag_name, r.region, tuple(tasks[t] for t in r.dtypes)) for r in engine.CALLER_INPUTS] == \
        [(name, kwarg, getattr(_lib, flag), 'DDP_' + flag, region, on) for name, kwarg, flag, region, on, _, _ in CC.ROWS]
    # a flag-clear engine has no map
    eng = object.__new__(DDPEngine)
    eng.cfg = S.make_cfg(dict(P.CASES['kc19_7x13_b3'], seed=1))
    for m in (eng.score_prior_view, eng.clear_score_prior, lambda: eng.set_score_prior(torch.zeros(1))):
        with pytest.raises(_lib.DdpError, match='score_prior=True'):
            m()
    eng.clear_score_prior(_if_any=True)


def test_plugin_surface_without_a_device():
    """``score_prior=None`` is a call-time argument of the seg plugin's entry points, the constructors stay the reference's, aug_test,
    slide inference and the FCN head raise, a map at another size is resized bilinearly, ``apis._run_batch`` moves a ``score_prior``
    entry like ``hints``"""
    import torch.nn.functional as F

    from ddp_amd import apis
    from ddp_amd.segmentors.ddp import DDP, SelfAlignedDDP
    assert 'score_prior' not in inspect.signature(DDP.__init__).parameters
    for m in ('ddim_sample', 'ddpm_sample', 'simple_test', 'forward', 'whole_inference', 'encode_decode', 'aug_test', 'slide_inference'):
        assert inspect.signature(getattr(DDP, m)).parameters['score_prior'].default is None, m
    assert inspect.signature(SelfAlignedDDP.self_aligned_predict).parameters['score_prior'].default is None
    assert inspect.signature(DDP._engine_for).parameters['score_prior'].default is False
    m = object.__new__(DDP)
    m.num_classes = 5
    dev = torch.device('cpu')
    for ac in (False, True):
        m.align_corners = ac
        same = torch.randn(2, 5, 3, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        t = DDP._score_prior_map(m, same, 2, 3, 4, dev)
        assert t.dtype == torch.float32 and t.is_contiguous() and torch.equal(t, same.float())
        big = torch.randn(2, 5, 12, 9, generator=torch.Generator().manual_seed(2))
        t = DDP._score_prior_map(m, big, 2, 3, 4, dev)
        assert torch.equal(t, F.interpolate(big, size=(3, 4), mode='bilinear', align_corners=ac)) and tuple(t.shape) == (2, 5, 3, 4)
    for bad in (torch.zeros(2, 4, 3, 4), torch.zeros(3, 5, 3, 4), torch.zeros(2, 5, 12), torch.zeros(2, 5, 3, 4, dtype=torch.int64),
                [torch.zeros(2, 5, 3, 4)], 'x'):
        with pytest.raises(ValueError, match='score_prior must be a float'):
            DDP._score_prior_map(m, bad, 2, 3, 4, dev)
    # the one forwarding helper: a None gives no key, a value exactly its key (prior and t_start travel together)
    assert m._given() == {} and m._given(0, 0) == {}
    for k, keys in (('hints', ['hints']), ('prior', ['prior', 't_start']), ('t_start', ['prior', 't_start']),
                    ('class_prior', ['class_prior']), ('score_prior', ['score_prior'])):
        assert list(m._given(**{k: same})) == keys and all(v is same or v is None for v in m._given(**{k: same}).values()), k
    # the refusals come before anything touches a device
    m.test_cfg = dict(mode='slide', crop_size=(8, 8), stride=(4, 4))
    img = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match='score_prior is not built for slide inference'):
        DDP.simple_test(m, img, None, score_prior=same)
    with pytest.raises(ValueError, match='score_prior is not built for slide inference'):
        DDP.slide_inference(m, img, None, False, score_prior=same)
    with pytest.raises(ValueError, match='score_prior is not built for aug_test'):
        DDP.aug_test(m, [img, img], [None, None], score_prior=same)
    seen = {}

    class _M(torch.nn.Module):
        def forward(self, **kw):
            seen.update(kw)
            return []
    apis._run_batch(_M(), dict(img=[torch.zeros(1, 3, 4, 4)], img_metas=[None], score_prior=torch.zeros(1, 5, 4, 4)), torch.device('cpu'))
    assert torch.is_tensor(seen['score_prior']) and seen['return_loss'] is False


def test_fcn_head_segmentor_raises():
    import ddp_amd
    from support import seg_cfg
    head = dict(type='FCNHeadWithTime', in_channels=256, channels=256, in_index=0, num_convs=1, num_classes=19, dropout_ratio=0.,
                norm_cfg=None, align_corners=False)
    model = ddp_amd.build_segmentor(seg_cfg(decode_head=head))
    with pytest.raises(ValueError, match="score_prior is built for the deformable head's sampler"):
        model._engine_for(1, 4, 4, torch.device('cpu'), 'ddim', score_prior=True)


def test_call_times_has_a_score_prior_variant():
    src = open(os.path.join(ROOT, 'scripts', 'call_times.py')).read()
    assert 'DDP_SCORE_PRIOR' in src and 'set_score_prior' in src and 'score_prior=True' in src
