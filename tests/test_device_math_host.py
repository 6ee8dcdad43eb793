"""CPU side of the device-math tests: the reference's own error budget, the folded GELU constants, the probe build (with its
compile-time checks of GELU_SCHED / SPLIT_HAND_LO) and the export lists of the two libraries."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import device_math_util as U
from ddp_amd import _lib, build
from support import dynamic_symbols as _dynamic_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_REF_CAP = 5e-7


def test_reference_budget():
    """E_ref = max |gelu_as_ref_f32 - gelu_exact| / |x| on dense + expo (|x| <= 64) stays under 5e-7.
    Derived budget per unit of |x|: A&S 7.1.26 truncation 0.5 x 1.5e-7, the fp32 polynomial and product about 0.5 x 1.5e-7,
    2^-24 for the final rounding = ~2.1e-7 .. 2.4e-7; the cap is twice that and FIXED, so that a drifting reference cannot widen
    the GPU bar (2 E_ref |x|, tests/test_device_math_gpu.py)."""
    ex = U.expo()
    x = np.concatenate([U.dense(), ex[np.abs(ex) <= 64]])
    e = U.e_ref(x)
    print(f'DEVICE-MATH E_ref (numpy float32 A&S 7.1.26 vs fp64 erf, {x.size} points) = {e:.3e} (cap {E_REF_CAP:.1e})')
    assert e <= E_REF_CAP
    assert e >= 0.5 * 1.5e-7 / 2      # sanity: an fp32 evaluation cannot be better than a fraction of the truncation error


def test_references_on_known_values():
    """the fp64 reference against values known in closed form; the split reference on hand-made patterns"""
    x = np.array([0.0, 1.0, -1.0, 3.0], dtype=np.float64)
    want = [0.0, 0.5 * (1 + math.erf(1 / math.sqrt(2))), -0.5 * (1 - math.erf(1 / math.sqrt(2))), 1.5 * (1 + math.erf(3 / math.sqrt(2)))]
    assert np.allclose(U.gelu_exact(x), want, rtol=1e-15, atol=0)
    v = np.array([0x3F812345, 0xBF800001, 0x3F800000, 0x7F7FFFFF], dtype=np.uint32).view(np.float32)
    p1, p2, p3 = U.cpu_split(v)
    assert [hex(b) for b in p1.view(np.uint32)] == ['0x3f810000', '0xbf800000', '0x3f800000', '0x7f7f0000']
    assert np.array_equal(U.sum3_f64(p1, p2, p3), v.astype(np.float64))
    for p in (p1, p2, p3):
        assert not np.any(p.view(np.uint32) & np.uint32(0xFFFF))
    # pack as the device does (perm 0x07060302: low half = element 2u, high half = element 2u + 1) and unpack again
    words = [(p.view(np.uint32)[0::2] >> 16) | (p.view(np.uint32)[1::2] & np.uint32(0xFFFF0000)) for p in (p1, p2, p3)]
    q1, q2, q3 = U.pieces_to_f32(*words)
    assert np.array_equal(q1, p1) and np.array_equal(q2, p2) and np.array_equal(q3, p3)


def test_grids():
    d, e, s, b = U.dense(), U.expo(), U.special(), U.bits()
    assert d.size == 2400001 and d[0] == np.float32(-12) and d[-1] == np.float32(12) and np.all(np.diff(d) > 0)
    assert e.size == 2 * 254 * 64 and np.all(np.isfinite(e)) and np.abs(e).min() >= 2.0 ** -126 and np.abs(e).max() >= 2.0 ** 127
    assert b.size == 1 << 20 and np.all(np.isfinite(b))
    sb = s.view(np.uint32)
    for pat in (0x0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000, 0x80800000, 0x1, 0x3F7FFFFF,
                0xBF800001, 0x3F810000, 0x3F800100):
        assert np.uint32(pat) in sb


def _folded_literals():
    src = open(os.path.join(build.CSRC, 'layer_bf16x3.h')).read()
    zp = re.search(r'constexpr double GELU_ZP = ([0-9.]+);', src)
    pz = re.search(r'constexpr double GELU_PZ = ([0-9.]+);', src)
    assert zp and pz, 'layer_bf16x3.h no longer names GELU_ZP / GELU_PZ'
    return src, float(zp.group(1)), float(pz.group(1))


def test_folded_gelu_constants():
    """z' = |x| sqrt(log2 e / 2) makes the A&S coefficient 0.3275911 / sqrt(log2 e): both folded constants are named once in
    layer_bf16x3.h, guarded there by a static_assert in double, and no second literal of either is left in the header."""
    src, zp, pz = _folded_literals()
    log2e = math.log2(math.e)
    assert abs(pz * math.sqrt(log2e) - 0.3275911) < 1e-9
    assert abs(2 * zp * zp - log2e) < 1e-15
    assert 'static_assert(gelu_cabs(GELU_PZ * 1.2011224087864498 - 0.3275911) < 1e-9' in src
    assert 'static_assert(gelu_cabs(2 * GELU_ZP * GELU_ZP - 1.4426950408889634) < 1e-15' in src
    assert abs(1.2011224087864498 - math.sqrt(log2e)) < 1e-15 and abs(1.4426950408889634 - log2e) < 1e-15
    # every use goes through the names: no other literal 0.2727.. / 0.8493.. in the header
    assert len(re.findall(r'0\.2727\d+', src)) == 1 and len(re.findall(r'0\.8493\d+', src)) == 1
    assert src.count('float(GELU_PZ)') == 3 and src.count('float(GELU_ZP)') == 2       # gelu_op<1>, <2>; gelu_split8_packed


@pytest.fixture(scope='module')
def probe_so(tmp_path_factory):
    """the probe compiled for gfx950 (no GPU needed); GELU_SCHED / SPLIT_HAND_LO are checked by static_assert in that TU"""
    out = str(tmp_path_factory.mktemp('probe') / 'libddp_probe.so')
    r = subprocess.run(build.probe_cmd(out), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_probe_builds_and_exports_only_probes(probe_so):
    syms = [s for s in _dynamic_symbols(probe_so) if not s.startswith('__hip_')]      # the fat-binary handles of every HIP object
    assert sorted(syms) == sorted(U.PROBE_EXPORTS), syms
    assert all(s.startswith('probe_') for s in syms)
    src = open(build.PROBE_SRC).read()
    for needle in ('static_assert(gelu_sched_ok()', 'static_assert(split_hand_ok()'):
        assert needle in src


def test_probe_compile_time_checks_reject_a_broken_schedule(tmp_path):
    """the static_asserts are live: a GELU_SCHED with two ops of one value swapped, and a SPLIT_HAND_LO that stops at 43, each
    fail the probe's compile (host pass only: -fsyntax-only, nothing is generated)."""
    hdr = open(os.path.join(build.CSRC, 'layer_bf16x3.h')).read()
    broken = {'sched': ('    { 9, 10,  8,  9},\n    {10, 11,  9, 10},', '    {10, 10,  8,  9},\n    { 9, 11,  9, 10},'),
              'hand': ('33, 38, 41, 44};', '33, 38, 41, 43};')}
    for name, (old, new) in broken.items():
        assert hdr.count(old) == 1
        csrc = tmp_path / name / 'ddp_amd' / 'csrc'          # the headers in the tree's layout (ddp_internal.h reaches ../../include)
        csrc.mkdir(parents=True)
        (tmp_path / name / 'include').mkdir()
        for h in build.HEADERS:
            if h.endswith('.h'):
                text = open(os.path.join(build.CSRC, h)).read()
                (csrc / h).write_text(text.replace(old, new) if h == 'layer_bf16x3.h' else text)
        cmd = [c if c != build.CSRC else str(csrc) for c in build.probe_cmd(str(tmp_path / name / 'x.so'))]
        cmd = [c for c in cmd if c != '-shared'] + ['-fsyntax-only', '--cuda-host-only']
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode != 0 and 'static assertion failed' in r.stderr, (name, r.stderr[-2000:])


def test_product_exports_unchanged():
    """libddp_mi355x.so still exports exactly _lib.EXPORTS (36 symbols): the probe is not part of the product"""
    build.build(verbose=False)
    syms = _dynamic_symbols(build.LIB_PATH)
    assert syms == sorted(_lib.EXPORTS) and len(syms) == 36
    assert not any('probe' in s for s in syms)
    # the package never loads the probe
    for dirpath, _, files in os.walk(os.path.join(ROOT, 'ddp_amd')):
        for f in files:
            if f.endswith('.py') and f != 'build.py':
                assert 'libddp_probe' not in open(os.path.join(dirpath, f)).read(), f


def test_probe_stamp_is_separate_from_the_product_hash(monkeypatch, tmp_path):
    """source_hash() covers SOURCES + HEADERS only; the probe has its own sha over its source + HEADERS"""
    import hashlib
    h = hashlib.sha256()
    for s in sorted(build.SOURCES + build.HEADERS):
        h.update(s.encode() + b'\0' + open(os.path.join(build.CSRC, s), 'rb').read())
    assert build.source_hash() == h.hexdigest()[:16]
    before = build.probe_hash()
    alt = tmp_path / 'device_math_probe.hip'
    alt.write_bytes(open(build.PROBE_SRC, 'rb').read() + b'\n')
    monkeypatch.setattr(build, 'PROBE_SRC', str(alt))
    assert build.probe_hash() != before and build.source_hash() == h.hexdigest()[:16]
