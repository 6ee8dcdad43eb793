"""CPU side of DDP_FLAG_DDPM_CHAIN (tests/test_ddpm_chain_gpu.py runs the cases on an MI355X): the oracle is well conditioned on
every case, the regrouped update is the reference's update, validate() accepts the flag where the header says and refuses it
elsewhere by message, the flag carves nothing, the flag-clear sizes are the parent build's, and the pre-pass kernel compiles for
gfx950 without scratch.  No GPU compute is invoked."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import config_space_cases as S
import ddpm_chain_cases as D
from ddp_amd import _lib
from golden_util import max_rel
from support import refused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'

FLAG_VARIANTS = [{}, dict(fused_tail=False), dict(nchw_head=False), dict(fused_layer=False), dict(fused_prologue=False)]


def test_flag_value_and_bars():
    assert _lib.FLAG_DDPM_CHAIN == 4096 and _lib.ABI_VERSION == 7 and len(_lib.EXPORTS) == 36
    assert D.REL == 2e-4 and D.COND == 1e-5 and D.CHAIN_VS_CLEAR == 5e-5
    with open(os.path.join(ROOT, 'include', 'ddp_mi355x.h')) as f:
        assert re.search(r'DDP_FLAG_DDPM_CHAIN = 4096\b', f.read())


@pytest.mark.parametrize('name', sorted(D.CASES))
def test_oracle_is_well_conditioned_on_the_case(name):
    """fp32 oracle vs its own fp64 evaluation: max-rel < COND = REL / 20 and identical decisions - the condition under which the
    suite's bar REL applies to the case unchanged.  (The two config-space ddpm cases are covered by test_config_space_host.py.)"""
    c = D.CASES[name]
    r32, r64 = D.oracle_batch(c, torch.float32), D.oracle_batch(c, torch.float64)
    assert r32.dtype == torch.float32 and r64.dtype == torch.float64 and r32.shape == (c['B'], c['Kc'], c['h'], c['w'])
    err = max_rel(r32.double(), r64)
    agree = float((r32.argmax(1) == r64.argmax(1)).float().mean())
    print(f'{name}: fp32 vs fp64 oracle max-rel {err:.2e} (cap {D.COND:.0e}), decisions equal {agree:.4f}')
    assert torch.isfinite(r64).all() and err < D.COND and agree == 1.0


@pytest.mark.parametrize('name', sorted(D.ALL))
def test_schedule_of_the_case(name):
    """the noise-adding steps of the table, the last step never among the pre-passes, and - dc_k2_td0: c == 1.0f exactly at step 0,
    so ua' == 0 there in fp32: the pre-pass must multiply, a form that divides by ua' does not exist"""
    c = D.ALL[name]
    recs = D.records(c)
    assert (D.prepasses(c), c['K']) == D.NOISE_STEPS[name]
    if name == 'dc_sr01':
        assert all(r['ddpm_add_noise'] for r in recs)             # the last step's flag is set - and must be ignored
    else:
        assert not recs[-1]['ddpm_add_noise']
    if name == 'dc_k2_td0':
        ua0, uc0 = D.chain_scalars(recs[0])
        assert np.float32(recs[0]['ddpm_c']) == np.float32(1.0) and ua0 == np.float32(0.0) and uc0 == np.float32(recs[0]['alpha_next'])
        assert recs[0]['ddpm_add_noise'] == 1                     # ... and that step does add noise: the pre-pass runs with ua' = 0
    for r in recs:
        ua, uc = D.chain_scalars(r)
        assert np.isfinite(ua) and np.isfinite(uc) and ua >= 0 and uc > 0


def test_small_ua_outside_the_first_step():
    """K = 10, sample_range0 = 0.3: a later step with ua' ~ 7e-4 - small factors are not confined to step 0"""
    recs = D.schedule.step_records('seg', 10, 1, 0.3, 'cosine', 'ddpm')
    uas = [float(D.chain_scalars(r)[0]) for r in recs]
    assert any(0 < u < 1e-3 for u in uas), uas


@pytest.mark.parametrize('name', sorted(D.ALL))
def test_regrouped_update_is_the_reference_update(name):
    """fp64 on random vectors, with the fp32 scalars the host hands over: W m' for m' = alpha' (m (1 - c) / alpha + c x0) + std eps
    (ddp.py:274-283) against ua' (W m) + uc' (W x0) + std (W eps).  The regrouping costs one fp32 rounding in ua' (two operations)
    and one in uc': |difference| <= 3 . 2^-24 . (|ua' u| + |uc' t|) per channel, and nothing on the noise term."""
    c = D.ALL[name]
    g = np.random.default_rng(c['seed'])
    W = g.standard_normal((256, 256)) / 16
    for r in D.records(c):
        m, x0, eps = g.standard_normal(256), (g.integers(0, 2, 256) * 2 - 1) * 0.01, g.standard_normal(256)
        cc, a, an, sd = (float(np.float32(r[k])) for k in ('ddpm_c', 'alpha', 'alpha_next', 'ddpm_std'))
        nz = eps if r['ddpm_add_noise'] else 0 * eps
        ref = W @ (an * (m * float(np.float32(1) - np.float32(cc)) / a + cc * x0) + sd * nz)
        ua, uc = (float(v) for v in D.chain_scalars(r))
        got = ua * (W @ m) + uc * (W @ x0) + sd * (W @ nz)
        bound = 3 * 2.0 ** -24 * (np.abs(ua) * np.abs(W) @ np.abs(m) + np.abs(uc) * np.abs(W) @ np.abs(x0)) + 1e-13
        assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())


@pytest.mark.parametrize('name', sorted(D.ALL))
def test_flag_is_accepted_and_carves_nothing(name):
    lib = _lib.load()
    c = D.ALL[name]
    for gemm in ('bf16x3', 'f32'):
        for fl in FLAG_VARIANTS:
            clear, chain = S.query(lib, D.make_cfg(c, False, gemm, **fl)), S.query(lib, D.make_cfg(c, True, gemm, **fl))
            assert clear[0] == 0 and chain[0] == 0, lib.ddp_last_error()
            assert chain == clear, (name, gemm, fl, clear, chain)
    for extra in (_lib.FLAG_RECORD_X0, _lib.FLAG_FORCE_X0, _lib.FLAG_STEP_RECORD, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_GATHER_GUESS_ZERO,
                  _lib.FLAG_STEP_RECORD | _lib.FLAG_SEEDED_NOISE | _lib.FLAG_RECORD_X0):
        a, b = D.make_cfg(c, False), D.make_cfg(c, True)
        a.flags |= extra
        b.flags |= extra
        qa, qb = S.query(lib, a), S.query(lib, b)
        assert qa[0] == 0 and qb == qa, (name, extra, lib.ddp_last_error())


# (total, model region) bytes of ddp_query_workspace / ddp_query_const_workspace for the flag-clear cfg of each case (bf16x3, default
# flags), recorded from the PARENT commit's build: the flag-clear carve is unchanged
PARENT_BYTES = {
    'dc_k2_td0': (31452928, 26034176), 'dc_15tok': (31391488, 25993216), 'dc_1x37_r2_cx96': (30750208, 24800000),
    'dc_1x257': (39175168, 26211840), 'dc_kc65_r2_nonoise': (39031808, 26199040), 'dc_kc256': (32630016, 26899968),
    'dc_k64': (32441088, 27054080), 'dc_L1': (23188480, 17774592), 'dc_sr01': (31469312, 26050560),
    'seg_ddpm_acc': (38686720, 26050560), 'seg_ddpm_noacc': (38686720, 26050560)}


@pytest.mark.parametrize('name', sorted(D.ALL))
def test_flag_clear_sizes_are_the_parent_builds(name):
    rc, total, model = S.query(_lib.load(), D.make_cfg(D.ALL[name], False))
    assert rc == 0 and (total, model) == PARENT_BYTES[name]


def test_flag_is_refused_elsewhere_by_message():
    lib = _lib.load()
    for name in ('seg_L12', 'seg_cx96_r2', 'depth_K1', 'depth_9x11_L1_bins', 'bev_kc8_r1', 'bev_kc9_r2'):     # seg + ddim, depth, bev
        for gemm in ('bf16x3', 'f32'):
            cfg = S.make_cfg(S.CASES[name], gemm)
            assert S.query(lib, cfg)[0] == 0
            cfg.flags |= _lib.FLAG_DDPM_CHAIN
            refused(lib, cfg, 'DDP_FLAG_DDPM_CHAIN exists for the segmentation ddpm sampler only')
    # the FCN loop: seg + ddpm is its configuration too, the flag is not
    import seeded_noise_util as U
    n = C.c_size_t(0)
    for flags in (0, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD):
        cfg = U.fcn_cfg(U.FCN_CASES['fcn_ddpm'], flags)
        assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == 0, lib.ddp_last_error()
        cfg.flags |= _lib.FLAG_DDPM_CHAIN
        assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == -1
        assert b'sample_fcn: DDP_FLAG_DDPM_CHAIN' in lib.ddp_last_error(), lib.ddp_last_error()
    cfg = U.fcn_cfg(U.FCN_CASES['fcn_ddim'], _lib.FLAG_DDPM_CHAIN)
    assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == -1
    assert b'DDP_FLAG_DDPM_CHAIN' in lib.ddp_last_error()
    # a bit nobody defines is still unknown
    cfg = D.make_cfg(D.CASES['dc_L1'])
    cfg.flags |= 8192
    refused(lib, cfg, 'unknown flags')


def test_plugin_attribute_and_engine_key():
    """``ddpm_chain`` is a class attribute (constructor kwargs stay the reference's) and part of the engine key"""
    import inspect

    from ddp_amd.segmentors.ddp import DDP, SelfAlignedDDP
    assert DDP.ddpm_chain is False and SelfAlignedDDP.ddpm_chain is False
    assert 'ddpm_chain' not in inspect.signature(DDP.__init__).parameters
    from ddp_amd.engine import DDPEngine
    assert inspect.signature(DDPEngine.__init__).parameters['ddpm_chain'].default is None
    from ddp_amd import build
    assert 'ddp_ddpm_chain.hip' in build.SOURCES


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_prepass_kernel_resources(tmp_path):
    """k_u_noise for gfx950: no scratch, the 32.5 KiB of LDS and at most 256 registers its header states (two waves per SIMD: the
    eight waves of a block on one CU), and the 128 fp32 MFMAs of one 32-token group x 32 channels per wave"""
    out = tmp_path / 'ddpm_chain.s'
    src = os.path.join(ROOT, 'ddp_amd', 'csrc', 'ddp_ddpm_chain.hip')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-x', 'hip', src,
                    '--cuda-device-only', '-S', '-o', str(out)], check=True, capture_output=True, timeout=600)
    text = out.read_text()
    found = re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', text, re.S)
    assert len(found) == 1 and 'k_u_noise' in found[0][0]
    body = found[0][1]
    assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0
    assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)) == 32 * 260 * 4
    assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 256
    assert len(re.findall(r'v_mfma_f32_32x32x2_f32', text)) == 128
