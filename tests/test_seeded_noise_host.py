"""DDP_FLAG_SEEDED_NOISE without a GPU: the NumPy restatement of the generator against Random123's known answers, the moment
conditions on the seed the GPU tests use, the workspace rule of include/ddp_mi355x.h and the unchanged ABI.  The compile-time
properties of the two fill kernels (byte-streaming: no LDS, no scratch) are checked here too."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import config_space_cases as S
import seeded_noise_util as U
from ddp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


def _hex(words):
    return ' '.join(f'{int(v):08x}' for v in words)


def test_restatement_reproduces_random123_known_answers():
    """philox4x32_10 of Random123's kat_vectors: counter / key all zero, all ones, and the digits of pi"""
    kat = [([0] * 4, [0] * 2, '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
           ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
           ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], 'd16cfe09 94fdcceb 5001e420 24126ea1')]
    for ctr, key, want in kat:
        got = U.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert _hex(got) == want, (ctr, key, _hex(got))


def test_restatement_is_vectorised_consistently():
    """a batch of counters gives, row by row, what single counters give; the pair radius belongs to lanes (0, 1) and (2, 3)"""
    z, rad = U.normals(U.SEED_B, 3, 2, 1, 10)
    one, _ = U.normals(U.SEED_B, 3, 2, 1, 3)
    assert np.array_equal(z[:3], one)
    assert rad[0] == rad[1] and rad[2] == rad[3] and rad[1] != rad[2]
    assert np.allclose(z[0] ** 2 + z[1] ** 2, rad[0] ** 2, rtol=1e-12)
    assert not np.array_equal(U.normals(U.SEED, 0, 0, 0, 8)[0], U.normals(U.SEED + (1 << 32), 0, 0, 0, 8)[0])     # the high key word counts


def test_uniforms_are_exact_in_fp32():
    """u = ((x >> 9) + 0.5) * 2^-23 is representable in fp32 at both ends, strictly inside (0, 1), and so is 2 u"""
    for x in (0, 1 << 9, 0xFFFFFFFF, 0x80000000):
        u = ((x >> 9) + 0.5) * 2.0 ** -23
        assert np.float32(u) == u and 0.0 < u < 1.0 and np.float32(2 * u) == 2 * u
        assert (np.float32(x >> 9) + np.float32(0.5)) * np.float32(2.0 ** -23) == u


def test_seed_of_the_gpu_tests_meets_the_moment_conditions():
    """a condition on the seed (picked on the CPU), not a measurement: n = 10^5, |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n)"""
    n = 100000
    z, rad = U.normals(U.SEED, 0, 0, 0, n)
    assert z.size == n and np.isfinite(z).all()
    print(f'SEEDED-NOISE seed {U.SEED}: mean {z.mean():+.5f} (bar {5 / np.sqrt(n):.5f}), var - 1 {z.var() - 1:+.5f} '
          f'(bar {5 * np.sqrt(2 / n):.5f}), max |z| {np.abs(z).max():.3f}, max rad {rad.max():.3f}')
    assert abs(z.mean()) <= 5 / np.sqrt(n)
    assert abs(z.var() - 1) <= 5 * np.sqrt(2 / n)
    assert np.abs(z).max() <= 5.77 and rad.max() <= 5.77        # sqrt(-2 ln(2^-24)) = 5.768


def _cfg(name, flags=0):
    c, f = U.CASES[name]
    kw = {k: v for k, v in f.items() if k != 'gemm'}
    cfg = S.make_cfg(c, f.get('gemm', 'bf16x3'), **kw)
    cfg.flags |= flags
    return c, cfg


@pytest.mark.parametrize('name', sorted(U.CASES))
def test_workspace_grows_by_the_noise_buffer_only(name):
    """ddp_query_workspace with the flag = the flagless value + round256(B r Cm h w 4), with and without DDP_FLAG_STEP_RECORD;
    ddp_query_const_workspace unchanged"""
    lib = _lib.load()
    c, plain = _cfg(name)
    rc, n0, m0 = S.query(lib, plain)
    assert rc == 0
    want = U.round256(c['B'] * c['r'] * U.cm_of(c) * c['h'] * c['w'] * 4)
    assert want == U.noise_bytes(c)
    _, seeded = _cfg(name, _lib.FLAG_SEEDED_NOISE)
    rc, n1, m1 = S.query(lib, seeded)
    assert rc == 0, lib.ddp_last_error().decode()
    assert n1 == n0 + want and m1 == m0
    _, rec = _cfg(name, _lib.FLAG_STEP_RECORD)
    _, both = _cfg(name, _lib.FLAG_STEP_RECORD | _lib.FLAG_SEEDED_NOISE)
    rc_r, nr, mr = S.query(lib, rec)
    rc_b, nb, mb = S.query(lib, both)
    assert rc_r == 0 and rc_b == 0
    assert nb == nr + want and mb == mr == m0


@pytest.mark.parametrize('name', sorted(U.FCN_CASES))
def test_fcn_workspace_grows_by_the_noise_buffer_only(name):
    lib = _lib.load()
    c = U.FCN_CASES[name]
    want = U.round256(c['B'] * c['r'] * 256 * c['h'] * c['w'] * 4)
    sizes = {}
    for flags in (0, _lib.FLAG_SEEDED_NOISE, _lib.FLAG_STEP_RECORD, _lib.FLAG_STEP_RECORD | _lib.FLAG_SEEDED_NOISE):
        n = C.c_size_t(0)
        cfg = U.fcn_cfg(c, flags)
        assert lib.ddp_sample_fcn_workspace(C.byref(cfg), c['num_convs'], 1, C.byref(n)) == 0, lib.ddp_last_error().decode()
        sizes[flags] = n.value
    assert sizes[_lib.FLAG_SEEDED_NOISE] == sizes[0] + want
    assert sizes[_lib.FLAG_STEP_RECORD | _lib.FLAG_SEEDED_NOISE] == sizes[_lib.FLAG_STEP_RECORD] + want


def test_flag_clear_gives_the_parents_workspace_sizes():
    """tests/golden/step_record/parent_workspace_bytes.json (recorded from the library before DDP_FLAG_STEP_RECORD) on every case of
    the configuration sweep: flag clear - the parent's numbers; flag set - the parent's total plus the formula, the parent's model
    region"""
    import json
    lib = _lib.load()
    golden = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'step_record', 'parent_workspace_bytes.json')))
    assert _lib.FLAG_SEEDED_NOISE == 2048
    for name, c in S.CASES.items():
        for vid, (gemm, fl) in {'bf16x3': ('bf16x3', {}), 'f32': ('f32', {})}.items():
            tot, const = golden['sample'][f'{name}/{vid}']
            assert list(S.query(lib, S.make_cfg(c, gemm, **fl))) == [0, tot, const], (name, vid)
            cfg = S.make_cfg(c, gemm, **fl)
            cfg.flags |= _lib.FLAG_SEEDED_NOISE
            assert list(S.query(lib, cfg)) == [0, tot + U.noise_bytes(c), const], (name, vid)
        if c['task'] == 'seg':
            for nc, dil in ((0, 1), (2, 1), (1, 2)):
                n = C.c_size_t(0)
                cfg = S.make_cfg(c)
                assert lib.ddp_sample_fcn_workspace(C.byref(cfg), nc, dil, C.byref(n)) == 0 and n.value == golden['fcn'][f'{name}/{nc}/{dil}']
                cfg.flags |= _lib.FLAG_SEEDED_NOISE
                assert lib.ddp_sample_fcn_workspace(C.byref(cfg), nc, dil, C.byref(n)) == 0
                assert n.value == golden['fcn'][f'{name}/{nc}/{dil}'] + U.noise_bytes(c)


def test_abi_is_unchanged_and_the_flag_is_accepted():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.ddp_abi_version() == 7
    assert len(_lib.EXPORTS) == 36
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in out.splitlines() if ' T ' in l and 'ddp_' in l)
    assert syms == sorted(_lib.EXPORTS)
    header = open(os.path.join(ROOT, 'include', 'ddp_mi355x.h')).read()
    assert re.search(r'DDP_FLAG_SEEDED_NOISE\s*=\s*2048', header) and '#define DDP_ABI_VERSION 7' in header
    for name in ('seg_fused', 'seg_ddpm', 'depth_chain', 'bev_chain'):
        for extra in (0, _lib.FLAG_STEP_RECORD, _lib.FLAG_UNFUSED_LAYER | _lib.FLAG_GATHER_GUESS_ZERO):
            _, cfg = _cfg(name, _lib.FLAG_SEEDED_NOISE | extra)
            n = C.c_size_t(0)
            assert lib.ddp_query_workspace(C.byref(cfg), C.byref(n)) == 0, (name, lib.ddp_last_error().decode())
    # the refusals of the other flags are unchanged
    _, cfg = _cfg('depth_chain', _lib.FLAG_SEEDED_NOISE | _lib.FLAG_RECORD_X0)
    assert lib.ddp_query_workspace(C.byref(cfg), C.byref(C.c_size_t(0))) == -1
    _, cfg = _cfg('seg_fused', _lib.FLAG_SEEDED_NOISE | _lib.FLAG_STEP_RECORD | _lib.FLAG_FORCE_X0)
    assert lib.ddp_query_workspace(C.byref(cfg), C.byref(C.c_size_t(0))) == -1
    _, cfg = _cfg('seg_fused', 4096)
    assert lib.ddp_query_workspace(C.byref(cfg), C.byref(C.c_size_t(0))) == -1 and b'unknown flags' in lib.ddp_last_error()


def test_key_words():
    from ddp_amd.engine import noise_key_words
    assert noise_key_words(U.SEED_B, 5, 2, 9) == [7, 0x12345678, 5, 2, 9, 0, 0, 0]
    assert noise_key_words(-1)[:2] == [0xFFFFFFFF, 0xFFFFFFFF]


def test_build_lists_the_generator_source():
    from ddp_amd import build
    assert 'ddp_noise.hip' in build.SOURCES


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_fill_kernels_are_byte_streaming(tmp_path):
    """k_noise_fill_nchw / k_noise_fill_tok: no LDS, no scratch, and few enough registers for eight waves per SIMD (<= 64); the
    accurate logf / sincospif are inlined library code, not the fast intrinsics (no v_log_f32 / v_sin_f32 on a raw argument would be
    hard to tell from assembly - the value test on the GPU is the check of that)"""
    out = tmp_path / 'noise.s'
    src = os.path.join(ROOT, 'ddp_amd', 'csrc', 'ddp_noise.hip')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-x', 'hip', src,
                    '--cuda-device-only', '-S', '-o', str(out)], check=True, capture_output=True, timeout=600)
    found = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', out.read_text(), re.S):
        body = m.group(2)
        found[m.group(1)] = (int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)),
                             int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)),
                             int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)))
    assert len(found) == 2 and any('k_noise_fill_nchw' in k for k in found) and any('k_noise_fill_tok' in k for k in found)
    for name, (scratch, lds, vgpr) in found.items():
        assert scratch == 0 and lds == 0, f'{name}: {scratch} B scratch, {lds} B LDS'
        assert vgpr <= 64, f'{name}: {vgpr} registers'
