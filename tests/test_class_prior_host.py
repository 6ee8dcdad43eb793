"""CPU side of DDP_FLAG_CLASS_PRIOR (tests/test_class_prior_gpu.py runs the cases on an MI355X): the expectation of
tests/class_prior_cases.py is the oracle's sampler on a biased state dict, reduces to the oracle's own result without a prior, is well
conditioned, takes decisions no fp32 rounding can flip (top-2 margin) and depends on the prior on every case; the flag's value, the
unchanged ABI, the workspace formulas, the unchanged flag-clear sizes, every refusal with its message, the compiled resources of the
kernels that changed and the device-free host surface.  No GPU compute is invoked."""
import ctypes as C
import inspect
import json
import os
import re
import shutil
import subprocess

import pytest
import torch

import class_prior_cases as P
import config_space_cases as S
from ddp_amd import _lib
from support import refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
FLAG_VARIANTS = [{}, dict(fused_tail=False), dict(nchw_head=False), dict(fused_layer=False), dict(fused_prologue=False)]
CASE_KINDS = [(n, k) for n in sorted(P.CASES) for k in P.KINDS]


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def test_flag_value_abi_and_bars():
    assert _lib.FLAG_CLASS_PRIOR == 131072 == 1 << 17 and _lib.ABI_VERSION == 7 and len(_lib.EXPORTS) == 36
    assert P.REL == 2e-4 and P.COND == 1e-5 and P.MARGIN == 1e-3 and P.WITNESS_PIXELS == 0.1 and P.CLAMP == 1e30
    header = open(os.path.join(ROOT, 'include', 'ddp_mi355x.h')).read()
    assert re.search(r'DDP_FLAG_CLASS_PRIOR\s*=\s*131072\b', header) and '#define DDP_ABI_VERSION 7' in header
    assert not re.search(r'=\s*8192\b', header) and not re.search(r'=\s*32768\b', header) and not re.search(r'=\s*262144\b', header)
    assert '/* class prior (DDP_FLAG_CLASS_PRIOR' in header
    lib = _lib.load()
    assert lib.ddp_abi_version() == 7
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in out.splitlines() if ' T ' in l and 'ddp_' in l)
    assert syms == sorted(_lib.EXPORTS) and len(syms) == 36
    assert C.sizeof(_lib.DdpCfg) == 136 and C.sizeof(_lib.DdpStep) == 32       # no struct grew
    from ddp_amd import build
    assert 'ddp_class_prior.hip' in build.SOURCES


def test_case_shapes():
    cs = P.CASES
    assert sorted(cs) == sorted(['kc19_7x13_b3', 'kc19_8x12_b2', 'kc150_9x14_noacc', 'kc255_5x10_r2', 'kc256_3x11', 'kc1_1x37_b3',
                                 'kc19_1x1_b3', 'ddpm_7x13'])
    geo = {n: (c['h'], c['w'], c['Kc'], c['B'], c['r']) for n, c in cs.items()}
    assert geo['kc19_7x13_b3'] == (7, 13, 19, 3, 1) and geo['kc19_8x12_b2'] == (8, 12, 19, 2, 1)
    assert geo['kc150_9x14_noacc'][:3] == (9, 14, 150) and not cs['kc150_9x14_noacc']['accumulation']
    assert geo['kc255_5x10_r2'] == (5, 10, 255, 2, 2) and geo['kc256_3x11'][2] == 256
    assert geo['kc1_1x37_b3'][:3] == (1, 37, 1) and geo['kc19_1x1_b3'] == (1, 1, 19, 3, 1)
    assert [c['sampler'] for c in cs.values()].count('ddpm') == 1
    for c in cs.values():
        assert c['K'] in (1, 2, 3) and c['L'] == 2 and c['task'] == 'seg'
    # image boundaries inside a 32-token tile / on tile boundaries / three images in one tile
    assert (7 * 13) % 32 != 0 and (8 * 12) % 32 == 0 and (2 * 5 * 10) % 32 != 0 and 3 * 1 < 32
    assert [n for n, c in cs.items() if not c['witness']] == ['kc1_1x37_b3']


@pytest.mark.parametrize('name,kind', CASE_KINDS)
def test_rows_hold_what_the_tests_need(name, kind):
    c = P.CASES[name]
    r = P.rows(c, kind)
    assert r.dtype == torch.float32 and tuple(r.shape) == (c['B'], c['Kc'])
    assert r.numpy().tobytes() == P.rows(c, kind).numpy().tobytes()                     # seeded
    for b in range(c['B'] - 1):                                                         # every image of a batch gets a different row
        assert c['Kc'] == 1 or not torch.equal(r[b], r[b + 1]) or kind == 'excl'
    if kind == 'soft':
        n = max(1, c['Kc'] // 3)
        for b in range(c['B']):
            assert int((r[b] != 0).sum()) == n and set(r[b][r[b] != 0].tolist()) <= {3.0, -3.0}
            assert c['Kc'] == 1 or bool((r[b] == 3.0).any())
    else:
        ex = P.excluded(c)
        for b in range(c['B']):
            assert sorted(torch.nonzero(torch.isinf(r[b])).flatten().tolist()) == ex[b] and bool((r[b][torch.isinf(r[b])] < 0).all())
            assert len(ex[b]) >= 1 and (c['Kc'] == 1 or len(ex[b]) < c['Kc'])
    odd = P.rows(c, 'odd')
    assert bool(torch.isnan(odd[:, 0]).all()) and (c['Kc'] <= 2 or (bool((odd == float('inf')).any()) and bool((odd == float('-inf')).any())))
    t = P.table(c, r)
    assert tuple(t.shape) == (c['B'], 256) and (c['Kc'] == 256 or bool(torch.isnan(t[:, c['Kc']:]).all()))
    cl = P.clamp(odd)
    big = float(torch.tensor(1e30, dtype=torch.float32))                               # (fl32(1e30) lies a little above 1e30)
    assert bool(torch.isfinite(cl).all()) and float(cl.max()) <= big and float(cl.min()) >= -big and bool((cl[:, 0] == 0).all())


@pytest.mark.parametrize('name', sorted(P.CASES))
def test_no_prior_is_the_oracles_sampler_bit_for_bit(name):
    """the expectation with a zero row == tests/config_space_cases.oracle_image (O.ddim_sample_seg / O.ddpm_sample_seg), torch.equal:
    fl32(bias + 0) is the bias, the ``head=`` hook that records the scores changes nothing"""
    for kind in P.KINDS:
        c = P.seeded(P.CASES[name], kind)
        e = P.expected(c, 'none')
        sd = S.state_dict(c)
        x, noise, sn = S.inputs(c)
        ref = torch.cat([S.oracle_image(c, sd, x, noise, sn, b) for b in range(c['B'])], 0)
        assert e['out'].dtype == torch.float32 and torch.equal(e['out'], ref)
        assert e['record'].shape == (c['K'], c['B'], c['r'], c['h'], c['w'])
        if not c['accumulation']:
            assert torch.equal(e['record'][-1, :, 0], ref.argmax(1).to(torch.uint8)) or c['r'] > 1


@pytest.mark.parametrize('name,kind', CASE_KINDS)
def test_expectation_is_well_conditioned_and_decides_with_margin(name, kind):
    """fp32 vs fp64 < COND = REL / 20 and the same decisions at every step; in fp64 the top-2 margin of every pixel at every step is
    >= 1e-3 of the step's largest score: no pixel is excused on the GPU.  (The seeds were chosen for this, see the case file.)"""
    c = P.CASES[name]
    e32, e64 = P.expected(c, kind), P.expected(c, kind, torch.float64)
    err = P.max_rel(e32['out'], e64['out'])
    print(f'CLASS-PRIOR {name}/{kind} seed {c["seeds"][kind]}: fp32 vs fp64 {err:.2e} (cap {P.COND:.0e}), fp64 top-2 margin '
          f'{e64["margin"]:.2e} (floor {P.MARGIN:.0e})')
    assert e64['out'].dtype == torch.float64 and torch.isfinite(e64['out']).all() and torch.isfinite(e32['out']).all()
    assert err < P.COND and torch.equal(e32['record'], e64['record'])
    assert e64['margin'] >= P.MARGIN and e32['margin'] >= P.MARGIN * 0.99


@pytest.mark.parametrize('name,kind', CASE_KINDS)
def test_the_prior_has_an_effect(name, kind):
    """witness: the prior changes the final decision on >= 10 % of the pixels of EACH image; the excluded classes held >= 10 % of the
    pixels without the prior and hold none with it - nor at any step.  (One class: one score channel, nothing to change.)"""
    c = P.CASES[name]
    base = P.final_decisions(c, 'none', seed_of=kind)
    e = P.expected(c, kind)
    fin = e['out'].argmax(1)
    changed = [float((fin[b] != base[b]).float().mean()) for b in range(c['B'])]
    line = f'CLASS-PRIOR {name}/{kind}: final decision changed on {min(changed):.2f} .. {max(changed):.2f} of the pixels'
    if not c['witness']:
        assert c['Kc'] == 1 and max(changed) == 0
        return
    assert min(changed) >= P.WITNESS_PIXELS, line
    if kind == 'excl':
        ex = P.excluded(c)
        for b in range(c['B']):
            held = sum(int((base[b] == k).sum()) for k in ex[b]) / base[b].numel()
            line += f'; image {b}: {ex[b]} held {held:.2f}'
            assert held >= P.WITNESS_PIXELS
            for k in ex[b]:
                assert int((fin[b] == k).sum()) == 0 and int((e['record'][:, b] == k).sum()) == 0
            if c['accumulation']:
                assert bool((e['out'][b, ex[b]] == 0).all())                 # softmax term exactly 0
            else:
                assert bool(torch.isfinite(e['out'][b]).all()) and float(e['out'][b, ex[b]].max()) <= -9e29
    print(line)


# ---- the C surface ------------------------------------------------------------------------------------------------------------------
def _with(cfg, flags):
    n = _lib.DdpCfg.from_buffer_copy(cfg)
    n.flags |= flags
    return n


def _extras(c):
    ex = [0, _lib.FLAG_STEP_RECORD, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD | _lib.FLAG_SEEDED_NOISE, _lib.FLAG_GATHER_GUESS_ZERO,
          _lib.FLAG_PRIOR_START, _lib.FLAG_PRIOR_START | _lib.FLAG_SEEDED_NOISE, _lib.FLAG_RECORD_X0, _lib.FLAG_FORCE_X0,
          _lib.FLAG_FORCE_X0 | _lib.FLAG_SEEDED_NOISE]
    if c['Kc'] < 256:
        ex += [_lib.FLAG_X0_HINTS, _lib.FLAG_X0_HINTS | _lib.FLAG_SEEDED_NOISE | _lib.FLAG_STEP_RECORD,
               _lib.FLAG_X0_HINTS | _lib.FLAG_PRIOR_START | _lib.FLAG_STEP_RECORD]
    if c['sampler'] == 'ddpm':
        ex += [_lib.FLAG_DDPM_CHAIN, _lib.FLAG_DDPM_CHAIN | _lib.FLAG_SEEDED_NOISE]
    return ex


@pytest.mark.parametrize('name', sorted(P.CASES))
def test_workspace_grows_by_the_documented_buffers_only(name):
    """ddp_query_workspace with the flag = the value without + round256(table_bytes) + round256(bias_bytes), under every other flag
    and both engines; ddp_query_const_workspace unchanged"""
    lib = _lib.load()
    c = P.seeded(P.CASES[name], 'soft')
    tb, bb = P.prior_bytes(c)
    assert tb == c['B'] * 256 * 4 and bb == 2 * tb
    for gemm in ('bf16x3', 'f32'):
        for fl in FLAG_VARIANTS:
            for extra in _extras(c):
                base = _with(S.make_cfg(c, gemm, **fl), extra)
                rc0, n0, m0 = S.query(lib, base)
                rc1, n1, m1 = S.query(lib, _with(base, _lib.FLAG_CLASS_PRIOR))
                assert rc0 == 0 and rc1 == 0, lib.ddp_last_error().decode()
                assert n1 == n0 + P.round256(tb) + P.round256(bb) and m1 == m0, (name, gemm, fl, extra)


def test_flag_clear_gives_the_parents_workspace_sizes():
    """tests/golden/step_record/parent_workspace_bytes.json (recorded from an earlier build) on every seg case of the configuration
    sweep it holds: flag clear - those numbers; flag set - that total plus the formulas, that model region"""
    lib = _lib.load()
    golden = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'step_record', 'parent_workspace_bytes.json')))
    seen = 0
    for name, c in S.CASES.items():
        for gemm in ('bf16x3', 'f32'):
            if f'{name}/{gemm}' not in golden['sample']:
                continue
            tot, const = golden['sample'][f'{name}/{gemm}']
            assert list(S.query(lib, S.make_cfg(c, gemm))) == [0, tot, const], (name, gemm)
            seen += 1
            if c['task'] == 'seg':
                tb, bb = P.prior_bytes(c)
                assert list(S.query(lib, _with(S.make_cfg(c, gemm), _lib.FLAG_CLASS_PRIOR))) == [0, tot + P.round256(tb) + P.round256(bb), const]
    assert seen > 60


def test_host_side_places_are_the_headers_formulas():
    """ddp_amd.engine.class_prior_places - the one host-side derivation - against the header's sentences, on a struct made without a
    device: the table immediately in front of the prior-start, hint, seeded-noise and step-record buffers, whichever exist, the
    library's vectors immediately in front of it, and every other offset the one of the cfg without the flag"""
    from ddp_amd.engine import class_prior_places, prior_start_places, step_record_sizes
    lib = _lib.load()
    for name in ('kc19_7x13_b3', 'kc255_5x10_r2', 'ddpm_7x13'):
        c = P.seeded(P.CASES[name], 'soft')
        tb, bb = P.prior_bytes(c)
        n = c['B'] * c['h'] * c['w']
        for extra in _extras(c):
            cfg = _with(S.make_cfg(c), extra | _lib.FLAG_CLASS_PRIOR)
            rc, total, _ = S.query(lib, cfg)
            assert rc == 0
            end = total
            if extra & _lib.FLAG_STEP_RECORD:
                rec, smap = step_record_sizes(cfg)
                end -= P.round256(rec) + P.round256(smap)
            if extra & _lib.FLAG_SEEDED_NOISE:
                end -= P.round256(n * c['r'] * 256 * 4)
            if extra & _lib.FLAG_X0_HINTS:
                end -= P.round256(n) + P.round256(n * c['r'])
            if extra & _lib.FLAG_PRIOR_START:
                end -= P.round256(n) + (0 if extra & _lib.FLAG_SEEDED_NOISE else P.round256(n * c['r'] * 256 * 4))
                po, pb, so, sb = prior_start_places(cfg, total)
                assert min(po, so) == end or (extra & _lib.FLAG_SEEDED_NOISE and po == end)
            table_at = end - P.round256(tb)
            assert class_prior_places(cfg, total) == (table_at, tb, table_at - P.round256(bb), bb), (name, extra)
            rc0, total0, _ = S.query(lib, _with(S.make_cfg(c), extra))
            trailing = total - end
            assert rc0 == 0 and table_at - P.round256(bb) == total0 - trailing


def test_refusals_carry_their_message():
    import prior_start_cases as PS
    lib = _lib.load()
    seg = P.seeded(P.CASES['kc19_7x13_b3'], 'soft')
    # depth and bev
    for other in ('depth_9x14', 'depth_1x37_bins', 'bev_kc8_r1', 'bev_kc9_r2'):
        base = S.make_cfg(PS.CASES[other])
        assert S.query(lib, base)[0] == 0
        refused(lib, _with(base, _lib.FLAG_CLASS_PRIOR), 'DDP_FLAG_CLASS_PRIOR')
    # the FCN loop: workspace query, prepare and sample
    import seeded_noise_util as U
    n = C.c_size_t(0)
    for case in ('fcn_ddim', 'fcn_ddpm'):
        for flags in (0, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD):
            cfg = U.fcn_cfg(U.FCN_CASES[case], flags)
            assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == 0, lib.ddp_last_error()
            cfg.flags |= _lib.FLAG_CLASS_PRIOR
            assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == -1
            assert b'sample_fcn: DDP_FLAG_CLASS_PRIOR' in lib.ddp_last_error(), lib.ddp_last_error()
            # ddp_sample_fcn / ddp_prepare_fcn validate before they touch a pointer
            assert lib.ddp_sample_fcn(C.byref(cfg), None, None, 1, 1, None, None, None, None, None, None, None) == -1
            assert b'sample_fcn: DDP_FLAG_CLASS_PRIOR' in lib.ddp_last_error(), lib.ddp_last_error()
            assert lib.ddp_prepare_fcn(C.byref(cfg), None, None, 1, 1, None, None, None) == -1
            assert b'sample_fcn: DDP_FLAG_CLASS_PRIOR' in lib.ddp_last_error(), lib.ddp_last_error()
    # bits 8192 and 32768 are still bits nobody defines, and so is every bit above the new one
    for bit in (8192, 32768, 262144, 1 << 19, 1 << 30):
        for extra in (bit, bit | _lib.FLAG_CLASS_PRIOR):
            refused(lib, _with(S.make_cfg(seg), extra), 'unknown flags')
    refused(lib, _with(S.make_cfg(PS.CASES['depth_9x14']), 262144), 'unknown flags')
    # what combines: every other flag of ddp_sample, 256 classes included
    for name in sorted(P.CASES):
        c = P.seeded(P.CASES[name], 'soft')
        for extra in _extras(c):
            assert S.query(lib, _with(S.make_cfg(c), extra | _lib.FLAG_CLASS_PRIOR))[0] == 0, (name, extra, lib.ddp_last_error())


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


@pytest.fixture(scope='module')
def compiled(tmp_path_factory):
    """{source: {kernel: (scratch bytes, registers, static LDS bytes)}} of the four translation units the flag touches, compiled side
    by side with the product's flags (one wall-clock compile for the whole file)"""
    from concurrent.futures import ThreadPoolExecutor
    tmp = str(tmp_path_factory.mktemp('class_prior_asm'))
    srcs = ['ddp_gemm_bf16.hip', 'ddp_layer_tail.hip', 'ddp_kernels.hip', 'ddp_class_prior.hip']
    with ThreadPoolExecutor(4) as ex:
        return dict(zip(srcs, ex.map(lambda s: _compile(tmp, s), srcs)))


# registers of the flag-clear (product) instantiations of the seg tails as the parent commit compiles them: k_layer<TAG, MODE, NCH, NT,
# FORCE = false>.  The class prior lives in the FORCE = true instantiations only, so these do not move
PARENT_VGPR = {'k_layerILi10ELi6ELi1ELb0ELb0E': 428, 'k_layerILi10ELi6ELi1ELb1ELb0E': 428, 'k_layerILi10ELi6ELi2ELb0ELb0E': 444,
               'k_layerILi10ELi6ELi2ELb1ELb0E': 444, 'k_layerILi10ELi6ELi3ELb0ELb0E': 444, 'k_layerILi10ELi6ELi3ELb1ELb0E': 444,
               'k_layerILi10ELi6ELi4ELb0ELb0E': 460, 'k_layerILi10ELi6ELi4ELb1ELb0E': 460,
               'k_layerILi8ELi1ELi1ELb0ELb0E': 284, 'k_layerILi8ELi1ELi2ELb0ELb0E': 316, 'k_layerILi8ELi1ELi3ELb0ELb0E': 437,
               'k_layerILi8ELi1ELi4ELb0ELb0E': 384, 'k_layerILi8ELi4ELi1ELb0ELb0E': 360, 'k_layerILi8ELi4ELi2ELb0ELb0E': 362,
               'k_layerILi8ELi4ELi3ELb0ELb0E': 362, 'k_layerILi8ELi4ELi4ELb0ELb0E': 389, 'k_layerILi3ELi3ELi0ELb0ELb0E': 352}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
@pytest.mark.parametrize('src', ['ddp_gemm_bf16.hip', 'ddp_layer_tail.hip'])
def test_layer_kernels_gain_no_scratch_and_the_product_tails_keep_their_registers(compiled, src):
    """every k_layer instantiation of the shipped code objects: no scratch, at most 512 registers; the flag-clear instantiations of the
    seg tails (and the 352-register projection kernel) hold exactly the parent's register count"""
    ks = {k: v for k, v in compiled[src].items() if 'k_layer' in k}
    assert len(ks) >= 18
    seen = 0
    for name, (scratch, vgpr, _) in ks.items():
        assert scratch == 0, f'{name}: {scratch} B of scratch'
        assert vgpr <= 512, name
        for key, want in PARENT_VGPR.items():
            if key in name:
                seen += 1
                assert vgpr == want, f'{name}: {vgpr} registers, the parent has {want}'
    assert seen >= 8
    forced = [n for n in ks if n.endswith('ELb0ELb1EEEvNS0_9LayerArgsE')]
    assert len(forced) in (4, 8)                                   # MODE 6 x 4 chunk counts; MODE 1 and 4 x 4


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_class_prior_and_seg_update_kernel_resources(compiled):
    """k_class_prior: no LDS, no scratch, <= 32 registers; k_seg_update: no scratch, no LDS, <= 64 registers (8 waves per SIMD)"""
    ks = compiled['ddp_class_prior.hip']
    assert len(ks) == 1
    (name, (scratch, vgpr, lds)), = ks.items()
    assert 'k_class_prior' in name and scratch == 0 and lds == 0 and vgpr <= 32
    upd = {k: v for k, v in compiled['ddp_kernels.hip'].items() if 'k_seg_update' in k}
    assert len(upd) == 1
    (scratch, vgpr, lds), = upd.values()
    print(f'k_seg_update: {vgpr} registers')
    assert scratch == 0 and lds == 0 and vgpr <= 64


# ---- host layer ---------------------------------------------------------------------------------------------------------------------
def test_engine_surface():
    from ddp_amd import engine
    from ddp_amd.engine import DDPEngine, FcnSamplerEngine, SampleGraph, class_mask_to_prior, class_prior_places
    assert inspect.signature(DDPEngine.__init__).parameters['class_prior'].default is False
    assert inspect.signature(FcnSamplerEngine.__init__).parameters['class_prior'].default is False
    for m in ('class_prior_view', 'set_class_prior', 'clear_class_prior'):
        assert callable(getattr(DDPEngine, m))
    assert inspect.signature(SampleGraph.replay).parameters['class_prior'].default is None
    with pytest.raises(ValueError, match='class_prior'):
        FcnSamplerEngine({}, None, h=4, w=4, class_prior=True)
    src = inspect.getsource(engine)
    assert src.index('def prior_start_places') < src.index('def class_prior_places') < src.index('def step_record_view')
    # a flag-clear engine has no table
    eng = object.__new__(DDPEngine)
    eng.cfg = S.make_cfg(P.seeded(P.CASES['kc19_7x13_b3'], 'soft'))
    for m in (eng.class_prior_view, eng.clear_class_prior):
        with pytest.raises(_lib.DdpError, match='class_prior'):
            m()
    eng.clear_class_prior(_if_any=True)
    # class_mask_to_prior: 0 where the class can occur, -inf where it cannot
    mask = torch.tensor([[True, False, True], [False, False, True]])
    pr = class_mask_to_prior(mask)
    assert pr.dtype == torch.float32 and torch.equal(pr == 0, mask) and torch.equal(torch.isinf(pr) & (pr < 0), ~mask)
    for bad in (mask.float(), mask[0], 'x'):
        with pytest.raises(ValueError, match='class_mask_to_prior'):
            class_mask_to_prior(bad)
    assert callable(class_prior_places)


def test_plugin_surface_without_a_device():
    """``class_prior=None`` is a call-time argument of the seg plugin's entry points, the constructors stay the reference's, the FCN head
    raises, ``apis._run_batch`` moves a ``class_prior`` entry like ``hints``"""
    from ddp_amd import apis
    from ddp_amd.segmentors.ddp import DDP, SelfAlignedDDP
    for k in ('class_prior',):
        assert k not in inspect.signature(DDP.__init__).parameters
    for m in ('ddim_sample', 'ddpm_sample', 'simple_test', 'forward', 'inference', 'aug_test', 'slide_inference'):
        assert inspect.signature(getattr(DDP, m)).parameters['class_prior'].default is None, m
    assert inspect.signature(SelfAlignedDDP.self_aligned_predict).parameters['class_prior'].default is None
    assert inspect.signature(DDP._engine_for).parameters['class_prior'].default is False
    m = object.__new__(DDP)
    m.num_classes = 5
    t = DDP._class_prior_table(m, torch.zeros(2, 5, dtype=torch.float64), 2, torch.device('cpu'))
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 5)
    rows = torch.arange(10.).view(2, 5)
    tiled = DDP._class_prior_table(m, rows, 2, torch.device('cpu'), repeat=3)          # window-major: row of map i = row of image i % b
    assert tuple(tiled.shape) == (6, 5) and all(torch.equal(tiled[i], rows[i % 2]) for i in range(6))
    for bad in (torch.zeros(2, 4), torch.zeros(3, 5), torch.zeros(5), torch.zeros(2, 5, dtype=torch.int64), [torch.zeros(2, 5)], 'x'):
        with pytest.raises(ValueError, match='class_prior'):
            DDP._class_prior_table(m, bad, 2, torch.device('cpu'))
    # the one forwarding helper: a None gives no key, a value exactly its key (prior and t_start travel together)
    assert m._given() == {} and m._given(0, 0) == {}
    for k, keys in (('hints', ['hints']), ('prior', ['prior', 't_start']), ('t_start', ['prior', 't_start']),
                    ('class_prior', ['class_prior']), ('score_prior', ['score_prior'])):
        assert list(m._given(**{k: rows})) == keys and all(v is rows or v is None for v in m._given(**{k: rows}).values()), k
    seen = {}

    class _M(torch.nn.Module):
        def forward(self, **kw):
            seen.update(kw)
            return []
    apis._run_batch(_M(), dict(img=[torch.zeros(1, 3, 4, 4)], img_metas=[None], class_prior=torch.zeros(1, 5)), torch.device('cpu'))
    assert torch.is_tensor(seen['class_prior']) and seen['return_loss'] is False


def test_fcn_head_segmentor_raises():
    import ddp_amd
    from support import seg_cfg
    head = dict(type='FCNHeadWithTime', in_channels=256, channels=256, in_index=0, num_convs=1, num_classes=19, dropout_ratio=0.,
                norm_cfg=None, align_corners=False)
    try:
        model = ddp_amd.build_segmentor(seg_cfg(decode_head=head))
    except Exception as e:                                                  # the FCN head's own constructor arguments
        pytest.fail(f'FCNHeadWithTime segmentor could not be built: {e}')
    with pytest.raises(ValueError, match='class_prior'):
        model._engine_for(1, 4, 4, torch.device('cpu'), 'ddim', class_prior=True)
