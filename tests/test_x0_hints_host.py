"""CPU side of DDP_FLAG_X0_HINTS (tests/test_x0_hints_gpu.py runs the cases on an MI355X): the hinted expectation of
tests/x0_hint_cases.py reduces to the oracle's own samplers where it must (bit for bit), is well conditioned and has an effect on
every case; the flag's value, the unchanged ABI, the two workspace formulas, the unchanged flag-clear sizes, every refusal with its
message, and the resources of the expand kernels.  No GPU compute is invoked."""
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
import x0_hint_cases as H
from ddp_amd import _lib
from oracle import ddp_oracle as O
from support import refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
FLAG_VARIANTS = [{}, dict(fused_tail=False), dict(nchw_head=False), dict(fused_layer=False), dict(fused_prologue=False)]


def test_flag_value_abi_and_bars():
    assert _lib.FLAG_X0_HINTS == 16384 and _lib.ABI_VERSION == 7 and len(_lib.EXPORTS) == 36
    assert H.REL == 2e-4 and H.COND == 1e-5 and H.WITNESS == 2e-3
    header = open(os.path.join(ROOT, 'include', 'ddp_mi355x.h')).read()
    assert re.search(r'DDP_FLAG_X0_HINTS\s*=\s*16384\b', header) and '#define DDP_ABI_VERSION 7' in header
    assert not re.search(r'=\s*8192\b', header)
    lib = _lib.load()
    assert lib.ddp_abi_version() == 7
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in out.splitlines() if ' T ' in l and 'ddp_' in l)
    assert syms == sorted(_lib.EXPORTS)
    assert C.sizeof(_lib.DdpCfg) == 136 and C.sizeof(_lib.DdpStep) == 32       # no struct grew
    from ddp_amd import build
    assert 'ddp_hints.hip' in build.SOURCES


def test_case_shapes():
    """B 2 or 3, token counts no multiple of 32, L = 2, K 3 or 4, seg class counts 1 / 19 / 150 / 255, one case without a witness"""
    assert {c['Kc'] for c in H.CASES.values() if c['task'] == 'seg'} == {1, 19, 150, 255}
    for c in H.CASES.values():
        assert c['B'] in (2, 3) and c['L'] == 2 and c['K'] in (3, 4) and (c['B'] * c['r'] * c['h'] * c['w']) % 32 != 0
    assert [n for n, c in H.CASES.items() if not c['witness']] == ['seg_kc1_1x37']
    assert {(c['h'], c['w']) for c in H.CASES.values()} >= {(7, 13), (9, 14), (5, 10), (1, 37), (1, 1)}


@pytest.mark.parametrize('name', sorted(H.CASES))
def test_free_hints_are_the_oracles_sampler_bit_for_bit(name):
    """the helper with every pixel free == O.ddim_sample_seg / O.ddpm_sample_seg / O.sample_depth (binned: the sampler of
    tests/depth_bins_util.py), torch.equal"""
    c = H.CASES[name]
    out, rec = H.expected(c, 'free')
    ref = S.oracle_batch(c)
    assert out.dtype == torch.float32 and out.shape == ref.shape and torch.equal(out, ref)
    assert rec.shape == (c['K'], c['B'], c['r'], c['h'], c['w'])


@pytest.mark.parametrize('name', H.names('seg', 'ddim'))
def test_full_hints_are_teacher_forcing_bit_for_bit(name):
    """every pixel hinted == O.ddim_sample_seg(x0_index = the hints at every step), torch.equal"""
    c = H.CASES[name]
    out, _ = H.expected(c, 'full')
    sd = S.state_dict(c)
    x, noise, _ = S.inputs(c)
    hints = H.full_hints(c)
    assert bool((hints < c['Kc']).all())
    for b in range(c['B']):
        idx = [hints[b][None].expand(c['r'], -1, -1)] * c['K']
        with torch.no_grad():
            ref = O.ddim_sample_seg(x[b:b + 1], noise[b], sd, timesteps=c['K'], randsteps=c['r'], bit_scale=c['bit_scale'],
                                    time_difference=c['td'], accumulation=c['accumulation'], x0_index=idx)
        assert torch.equal(out[b:b + 1], ref), (name, b)


@pytest.mark.parametrize('kind', ['partial', 'full'])
@pytest.mark.parametrize('name', sorted(H.CASES))
def test_hinted_expectation_is_well_conditioned(name, kind):
    """fp32 helper vs its own fp64 evaluation < COND = REL / 20 (as tests/config_space_cases.py requires of every case), and - seg -
    the model's own decisions agree at every step: the condition under which REL applies to the GPU comparison unchanged"""
    c = H.CASES[name]
    (o32, r32), (o64, r64) = H.expected(c, kind, torch.float32), H.expected(c, kind, torch.float64)
    err = H.max_rel(o32, o64)
    print(f'{name}/{kind}: fp32 vs fp64 max-rel {err:.2e} (cap {H.COND:.0e})')
    assert o64.dtype == torch.float64 and torch.isfinite(o64).all() and err < H.COND
    if c['task'] == 'seg':
        assert torch.equal(r32, r64)
    else:
        assert H.max_rel(r32, r64) < H.COND


@pytest.mark.parametrize('kind', ['partial', 'full'])
@pytest.mark.parametrize('name', sorted(H.CASES))
def test_hints_have_an_effect(name, kind):
    """witness: the hinted expectation differs from the unhinted one by more than 10 * REL - a GPU result within REL of it cannot be
    the unhinted sampler's.  (One class: the only hint is the argmax - no effect possible, stated in the cases file.)"""
    c = H.CASES[name]
    d = H.max_rel(H.expected(c, kind)[0], H.expected(c, 'free')[0])
    print(f'{name}/{kind}: hinted vs free max-rel {d:.2e}')
    if c['witness']:
        assert d > H.WITNESS
    else:
        assert c['Kc'] == 1 and d == 0.0


@pytest.mark.parametrize('name', sorted(H.CASES))
def test_partial_hint_maps_hold_what_the_tests_need(name):
    c = H.CASES[name]
    hints = H.partial_hints(c)
    N = c['h'] * c['w']
    on = torch.stack([H.hinted(c, hints[b]) for b in range(c['B'])]).view(c['B'], N)
    assert on.any() and (N == 1 or not on.all())
    if c['task'] == 'seg':
        assert hints.dtype == torch.uint8
        free = hints.view(c['B'], N)[~on]
        assert bool((free >= c['Kc']).all()) and (c['Kc'] >= 254 or N == 1 or len(set(free.tolist())) > 1)      # several free encodings
        assert bool(on[:, 0].all()) and bool(on[:, -1].all())        # the block runs over the border between image b and b + 1
    else:
        assert hints.dtype == torch.float32
        flat = hints.view(-1)
        if N > 1:
            assert torch.isnan(flat).any() and torch.isinf(flat).any() and (flat < 0).any() and (flat == 0).any()
            assert ((flat > 0) & (flat < c['min_depth'])).any() and (torch.isfinite(flat) & (flat > c['max_depth'])).any()


def _with(cfg, flags):
    n = _lib.DdpCfg.from_buffer_copy(cfg)
    n.flags |= flags
    return n


@pytest.mark.parametrize('name', sorted(H.CASES))
def test_workspace_grows_by_the_two_buffers_only(name):
    """ddp_query_workspace with the flag = the value without + round256(hint_bytes) + round256(row_bytes), for every combination with
    DDP_FLAG_STEP_RECORD / DDP_FLAG_SEEDED_NOISE, every route flag and both engines; ddp_query_const_workspace unchanged"""
    lib = _lib.load()
    c = H.CASES[name]
    hb, rb = H.hint_bytes(c)
    assert hb == c['B'] * c['h'] * c['w'] * (1 if c['task'] == 'seg' else 4) and rb == hb * c['r']
    want = H.round256(hb) + H.round256(rb)
    for gemm in ('bf16x3', 'f32'):
        for fl in FLAG_VARIANTS:
            for extra in (0, _lib.FLAG_STEP_RECORD, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD | _lib.FLAG_SEEDED_NOISE):
                base = _with(S.make_cfg(c, gemm, **fl), extra)
                rc0, n0, m0 = S.query(lib, base)
                rc1, n1, m1 = S.query(lib, _with(base, _lib.FLAG_X0_HINTS))
                assert rc0 == 0 and rc1 == 0, lib.ddp_last_error().decode()
                assert n1 == n0 + want and m1 == m0, (name, gemm, fl, extra)
    if c['task'] == 'seg':
        for extra in (_lib.FLAG_RECORD_X0, _lib.FLAG_GATHER_GUESS_ZERO) + ((_lib.FLAG_DDPM_CHAIN,) if c['sampler'] == 'ddpm' else ()):
            base = _with(S.make_cfg(c), extra)
            (rc0, n0, m0), (rc1, n1, m1) = S.query(lib, base), S.query(lib, _with(base, _lib.FLAG_X0_HINTS))
            assert rc0 == 0 and rc1 == 0 and n1 == n0 + want and m1 == m0


def test_flag_clear_gives_the_parents_workspace_sizes():
    """tests/golden/step_record/parent_workspace_bytes.json (recorded from an earlier build) on every seg / depth case of the
    configuration sweep: flag clear - those numbers; flag set - that total plus the two formulas, that model region"""
    lib = _lib.load()
    golden = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'step_record', 'parent_workspace_bytes.json')))
    seen = 0
    for name, c in S.CASES.items():
        if c['task'] == 'bev':
            continue
        hb, rb = H.hint_bytes(c)
        for gemm in ('bf16x3', 'f32'):
            tot, const = golden['sample'][f'{name}/{gemm}']
            assert list(S.query(lib, S.make_cfg(c, gemm))) == [0, tot, const], (name, gemm)
            assert list(S.query(lib, _with(S.make_cfg(c, gemm), _lib.FLAG_X0_HINTS))) == [0, tot + H.round256(hb) + H.round256(rb), const]
            seen += 1
    assert seen > 60


def test_refusals_carry_their_message():
    lib = _lib.load()
    # bev
    for name in ('bev_kc8_r1', 'bev_kc9_r2'):
        for gemm in ('bf16x3', 'f32'):
            cfg = S.make_cfg(S.CASES[name], gemm)
            assert S.query(lib, cfg)[0] == 0
            refused(lib, _with(cfg, _lib.FLAG_X0_HINTS), 'DDP_FLAG_X0_HINTS', 'bev')
    # together with teacher forcing
    cfg = S.make_cfg(H.CASES['seg_kc19_7x13'])
    assert S.query(lib, _with(cfg, _lib.FLAG_FORCE_X0))[0] == 0
    refused(lib, _with(cfg, _lib.FLAG_X0_HINTS | _lib.FLAG_FORCE_X0), 'DDP_FLAG_X0_HINTS', 'DDP_FLAG_FORCE_X0')
    # seg with 256 classes: accepted without the flag, and 255 with it
    c256 = dict(H.CASES['seg_kc255_5x10_r2'], Kc=256)
    assert S.query(lib, S.make_cfg(c256))[0] == 0
    refused(lib, _with(S.make_cfg(c256), _lib.FLAG_X0_HINTS), 'DDP_FLAG_X0_HINTS', '256')
    assert S.query(lib, _with(S.make_cfg(H.CASES['seg_kc255_5x10_r2']), _lib.FLAG_X0_HINTS))[0] == 0
    # depth does not look at num_classes
    assert S.query(lib, _with(S.make_cfg(dict(H.CASES['depth_9x14'], Kc=256)), _lib.FLAG_X0_HINTS))[0] == 0
    # the FCN loop and its workspace query
    import seeded_noise_util as U
    n = C.c_size_t(0)
    for case in ('fcn_ddim', 'fcn_ddpm'):
        for flags in (0, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD):
            cfg = U.fcn_cfg(U.FCN_CASES[case], flags)
            assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == 0, lib.ddp_last_error()
            cfg.flags |= _lib.FLAG_X0_HINTS
            assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == -1
            assert b'sample_fcn: DDP_FLAG_X0_HINTS' in lib.ddp_last_error(), lib.ddp_last_error()
            # ddp_sample_fcn / ddp_prepare_fcn validate before they touch a pointer
            assert lib.ddp_sample_fcn(C.byref(cfg), None, None, 1, 1, None, None, None, None, None, None, None) == -1
            assert b'sample_fcn: DDP_FLAG_X0_HINTS' in lib.ddp_last_error(), lib.ddp_last_error()
    # bit 8192 is still a bit nobody defines
    for extra in (8192, 8192 | _lib.FLAG_X0_HINTS):
        refused(lib, _with(S.make_cfg(H.CASES['seg_kc19_7x13']), extra), 'unknown flags')
    refused(lib, _with(S.make_cfg(H.CASES['depth_9x14']), 32768), 'unknown flags')


def test_engine_and_plugin_surface():
    """constructor keywords and methods of the host layer (no device needed to read them)"""
    from ddp_amd.engine import DDPEngine, FcnSamplerEngine, SampleGraph
    assert inspect.signature(DDPEngine.__init__).parameters['x0_hints'].default is False
    assert inspect.signature(FcnSamplerEngine.__init__).parameters['x0_hints'].default is False
    for m in ('hints_view', 'set_hints', 'clear_hints'):
        assert callable(getattr(DDPEngine, m))
    assert inspect.signature(SampleGraph.replay).parameters['hints'].default is None
    with pytest.raises(ValueError, match='x0_hints'):
        FcnSamplerEngine({}, None, h=4, w=4, x0_hints=True)


def test_plugin_surface_without_a_device():
    """``hints=None`` is a call-time argument of the plugin classes, their constructors stay the reference's; the bev class, aug_test
    and slide inference raise ValueError when given hints; ``hints`` is part of the engine key"""
    from ddp_amd import apis
    from ddp_amd.bev.ddp import DDP as BevDDP
    from ddp_amd.depther.ddp import DDP as DepthDDP
    from ddp_amd.segmentors.ddp import DDP as SegDDP
    for cls, methods in ((SegDDP, ('ddim_sample', 'ddpm_sample', 'simple_test', 'forward', 'aug_test', 'slide_inference')),
                         (DepthDDP, ('sample', 'simple_test', 'inference', 'aug_test')), (BevDDP, ('ddim_sample',))):
        assert 'hints' not in inspect.signature(cls.__init__).parameters
        for m in methods:
            assert inspect.signature(getattr(cls, m)).parameters['hints'].default is None, (cls, m)
    assert inspect.signature(SegDDP._engine_for).parameters['hints'].default is False
    with pytest.raises(ValueError, match='hints'):
        BevDDP.ddim_sample(object.__new__(BevDDP), [torch.zeros(1)], None, hints=torch.zeros(1, 2, 2))
    for cls in (SegDDP, DepthDDP):
        with pytest.raises(ValueError, match='hints'):
            cls.aug_test(object.__new__(cls), [None, None], [None, None], hints=torch.zeros(1, 2, 2))
    with pytest.raises(ValueError, match='hints'):
        SegDDP.slide_inference(object.__new__(SegDDP), None, None, False, hints=torch.zeros(1, 2, 2))
    # nearest resampling to the map, the rule of segmentors/ddp.py:149, at a non-integer ratio; holes are not averaged
    src = torch.zeros(2, 7, 9)
    src[:, 3, 4] = 50.0
    m = SegDDP._hint_map([src], 2, 3, 4, torch.float32)
    assert tuple(m.shape) == (2, 3, 4) and set(m.unique().tolist()) <= {0.0, 50.0}
    assert torch.equal(m, torch.nn.functional.interpolate(src[:, None], size=(3, 4), mode='nearest')[:, 0])
    assert SegDDP._hint_map(torch.full((2, 7, 9), 255, dtype=torch.uint8), 2, 3, 4, torch.uint8).dtype == torch.uint8
    for bad in (torch.zeros(3, 7, 9), torch.zeros(7, 9), [src, src], 'x'):
        with pytest.raises(ValueError, match='hints'):
            SegDDP._hint_map(bad, 2, 3, 4, torch.uint8)
    # the harness hands a ``hints`` entry of the batch through, on the model's device
    seen = {}

    class _M(torch.nn.Module):
        def forward(self, **kw):
            seen.update(kw)
            return []
    apis._run_batch(_M(), dict(img=[torch.zeros(1, 3, 4, 4)], img_metas=[None], hints=[torch.zeros(1, 4, 4)]), torch.device('cpu'))
    assert torch.is_tensor(seen['hints'][0]) and seen['return_loss'] is False


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_expand_kernel_resources(tmp_path):
    """k_hint_rows_seg / k_hint_rows_depth for gfx950: byte-streaming - no LDS, no scratch, <= 64 registers"""
    out = tmp_path / 'hints.s'
    src = os.path.join(ROOT, 'ddp_amd', 'csrc', 'ddp_hints.hip')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-x', 'hip', src,
                    '--cuda-device-only', '-S', '-o', str(out)], check=True, capture_output=True, timeout=600)
    found = re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', out.read_text(), re.S)
    assert len(found) == 2 and any('k_hint_rows_seg' in n for n, _ in found) and any('k_hint_rows_depth' in n for n, _ in found)
    for name, body in found:
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 64, name
