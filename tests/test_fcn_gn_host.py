"""CPU companion of tests/test_fcn_gn_gpu.py (cases and expectation: tests/fcn_gn_cases.py): the expectation is well conditioned, every
case does what its name says, the reference fixtures are the expectation bit for bit, the plugin surface without a device, nothing of
the C ABI moved (version, exports, both workspace queries), the new kernel's resources, and the drop-in check in the reference's
own registry."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

import fcn_gn_cases as G
from ddp_amd import _lib
from support import max_rel64 as _rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
import ref_shim  # noqa: E402


def test_bars():
    from support import REL
    assert G.REL == REL == 2e-4 and G.F32_VS_F64 == 1e-5 and G.MARGIN == 1e-3 and G.MARGIN >= 5 * G.REL


# ---- the expectation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(G.HEAD))
def test_head_expectation_fp32_vs_fp64(name):
    c = G.HEAD[name]
    e = _rel(G.head_expect(c), G.head_expect(c, torch.float64))
    print(f'FCN-GN head {name}: fp32 vs fp64 expectation {e:.2e}')
    assert e < G.F32_VS_F64


@pytest.mark.parametrize('name', list(G.LOOP))
def test_loop_expectation_fp32_vs_fp64_and_margin(name):
    """fp32 within 1e-5 of fp64; the fp64 expectation's top-2 margin is at least 1e-3 of the step's largest |score| at every pixel
    and step, so both precisions (and any implementation within REL) take the same decisions"""
    c = G.LOOP[name]
    o32, s32 = G.loop_expect(c)
    o64, s64 = G.loop_expect(c, torch.float64)
    e, m = _rel(o32, o64), G.loop_min_margin(s64)
    print(f'FCN-GN loop {name}: fp32 vs fp64 {e:.2e}, smallest top-2 margin {m:.2e}')
    assert e < G.F32_VS_F64 and m >= G.MARGIN
    assert torch.equal(G.loop_decisions(s32), G.loop_decisions(s64))
    assert G.loop_decisions(s32).shape == (c['K'], c['B'], c['r'], c['h'], c['w'])


def _taps(c):
    feat, temb = G.head_inputs(c)
    seen = []
    with torch.no_grad():
        G.expect_head(feat.double(), temb.double() if temb is not None else None, G.cast(G.head_state(c), torch.float64), c['num_convs'],
                      c['dilation'], c['eps'], tap=lambda i, y, n: seen.append((y, n)))
    return seen


@pytest.mark.parametrize('name', list(G.HEAD))
def test_head_case_does_what_its_name_says(name):
    c = G.HEAD[name]
    sd = G.head_state(c)
    N, M = c['h'] * c['w'], c['maps'] * c['h'] * c['w']
    assert len(c['norms']) == c['num_convs']
    for i, kind in enumerate(c['norms']):
        p = f'convs.{i}.'
        assert (p + 'gn.weight' in sd) == (kind == 'gn') and (p + 'bn.running_var' in sd) == (kind == 'bn')
        assert (p + 'conv.bias' in sd) == (kind is None or (kind == 'gn' and c['conv_b']))
    taps = _taps(c)
    for (y, n), kind in zip(taps, c['norms']):
        if kind != 'gn':
            continue
        g = y.reshape(c['maps'], 32, 8 * N)
        mean, var = g.mean(2), g.var(2, unbiased=False)
        # the statistics are per map: normalising with them centres every (map, group) ...
        z = (g - mean[..., None]) / (var[..., None] + c['eps']).sqrt()
        assert torch.allclose(z.mean(2), torch.zeros_like(mean), atol=1e-9)
        # ... and they differ between the maps: pooling them would be another tensor
        if c['maps'] > 1:
            assert float((mean[0] - mean[1]).abs().max()) > 1e-3 or float((var[0] - var[1]).abs().max()) > 1e-3
        if c['conv_b']:
            assert float(mean.abs().mean()) > 0.05               # the bias is inside the statistics (0.2 + 0.3 randn)
    if name.startswith('pixel'):
        assert N == 1 and not G.fused_route(c)                   # 8 values per group
    if name == 'pixels_5':
        assert c['maps'] > 2 and M <= G.APPLY_BLOCK              # a third map inside one block of the apply pass
    if name in ('row_1x37', 'col_37x1', 'odd_3maps', 'notime_d2', 'gamma_zeros', 'mixed_gn_bn'):
        assert not G.fused_route(c)
    if name == 'odd_3maps':
        assert c['maps'] == 3 and M <= G.APPLY_BLOCK and M % 32
    if name.startswith('wave_4x8'):
        assert N == 32 and G.fused_route(c)                      # exactly one wave per map
    if name == 'wave_4x8_d3':
        assert c['dilation'] == 3 and c['dilation'] >= c['h'] - 1   # vertical taps reach at most the opposite border row
    if name == 'waves_8x8':
        assert N == 64 and G.fused_route(c) and c['eps'] == 1e-3
    if name == 'tiles_24x24':
        assert G.fused_route(c) and M > 256 * 6 and N % 256 and N % G.APPLY_BLOCK   # map borders inside tiles and apply blocks
    if name == 'eight_convs':
        assert c['num_convs'] == 8
    if name == 'no_convs':
        assert c['num_convs'] == 0 and not taps
    if name == 'notime_d2':
        assert G.head_inputs(c)[1] is None and c['dilation'] == 2
    if name == 'gamma_zeros':
        ga = sd['convs.0.gn.weight']
        assert int((ga == 0).sum()) >= 50 and float(ga.min()) < -1 and bool((ga[8:16] == 0).all())
    if name == 'mixed_bn_gn_none':
        assert c['norms'] == ('bn', 'gn', None)
    assert sorted({c['classes'] for c in G.HEAD.values()}) == [1, 19, 150, 256]
    assert {c['dilation'] for c in G.HEAD.values()} == {1, 2, 3} and {c['num_convs'] for c in G.HEAD.values()} >= {0, 1, 2, 8}
    assert {c['eps'] for c in G.HEAD.values()} == {1e-5, 1e-3}


def test_loop_cases_cover_what_they_should():
    br = {(c['B'], c['r']) for c in G.LOOP.values()}
    assert {(1, 1), (2, 2)} <= br and ((2, 1) in br or (1, 2) in br)
    assert {c['sampler'] for c in G.LOOP.values()} == {'ddim', 'ddpm'}
    assert {G.fused_route(c) for c in G.LOOP.values()} == {True, False}
    assert G.LOOP['r2_ddpm_mixed']['norms'] == ('bn', 'gn')


def test_eps_has_an_effect():
    """eps 1e-3 is visible at REL: a library that ignored bn_eps would miss the bar"""
    c = G.HEAD['waves_8x8']
    other = dict(c, eps=1e-5, name='waves_8x8_other_eps')
    assert _rel(G.head_expect(other), G.head_expect(c)) > G.REL


# ---- the reference fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', G.FIXTURE_HEADS)
def test_reference_head_fixture_is_the_expectation_bit_for_bit(name):
    c, feat, temb, sd, ref = G.load_fixture_head(name)
    with torch.no_grad():
        out = G.expect_head(feat, temb.expand(c['maps'], 1024) if temb is not None else None, sd, c['num_convs'], c['dilation'], c['eps'])
    assert torch.equal(out, ref)


@pytest.mark.parametrize('name', G.FIXTURE_LOOPS)
def test_reference_loop_fixture_is_the_expectation_bit_for_bit(name):
    c, sd, x, noise, sn, ref, logits = G.load_fixture_loop(name)
    out, steps = G.run_loop(c, sd, x, noise, sn)
    assert torch.equal(out, ref) and torch.equal(torch.stack(steps[0]), logits)


# ---- plugin surface without a device -------------------------------------------------------------------------------------------
def test_plugin_surface_without_a_device():
    import ddp_amd
    from ddp_amd.utils import synthetic
    head = ddp_amd.FCNHeadWithTime(num_convs=2, concat_input=True, in_channels=256, channels=256, num_classes=19,
                                   norm_cfg=dict(type='GN', num_groups=32))
    sd = synthetic.make_fcn_state_dict(2, 19, True, True, 3, norm='gn')
    assert set(head.state_dict()) == set(sd) and {'convs.0.gn.weight', 'convs.1.gn.bias', 'conv_cat.gn.weight', 'conv_cat.gn.bias'} <= set(sd)
    assert not any('bn.' in k or k.endswith('conv.bias') for k in sd if k.startswith('convs.'))
    head.load_state_dict(sd, strict=True)
    assert isinstance(head.convs[0].gn, torch.nn.GroupNorm) and head.convs[0].gn.num_groups == 32 and head.convs[0].gn.eps == 1e-5
    arr, keep = head.conv_array()
    for i in range(2):
        assert arr[i].bn_w and arr[i].bn_b and not arr[i].bn_mean and not arr[i].bn_var and arr[i].conv_w and not arr[i].conv_b
        assert arr[i].bn_eps == pytest.approx(1e-5) and arr[i].time_w and arr[i].time_b
    assert ddp_amd.FCNHeadWithTime(num_convs=1, norm_cfg=dict(type='GN', num_groups=32, eps=1e-3)).conv_array()[0][0].bn_eps == pytest.approx(1e-3)
    for bad in (dict(type='GN', num_groups=16), dict(type='LN'), dict(type='GN')):
        with pytest.raises(NotImplementedError, match='num_groups=32'):
            ddp_amd.FCNHeadWithTime(num_convs=1, norm_cfg=bad)
    # BatchNorm and norm-free heads: the parent's pattern
    arr, _ = ddp_amd.FCNHeadWithTime(num_convs=1, norm_cfg=dict(type='BN')).conv_array()
    assert arr[0].bn_w and arr[0].bn_b and arr[0].bn_mean and arr[0].bn_var and not arr[0].conv_b
    arr, _ = ddp_amd.FCNHeadWithTime(num_convs=1, norm_cfg=None).conv_array()
    assert not arr[0].bn_w and not arr[0].bn_b and arr[0].conv_b
    # today's callers of make_fcn_state_dict pass with_norm positionally and get BatchNorm keys
    assert 'convs.0.bn.running_mean' in synthetic.make_fcn_state_dict(1, 19, True, False, 0)
    with pytest.raises(_lib.DdpError, match='CUDA'):
        head.eval()([torch.zeros(1, 256, 4, 8)], None)


def test_segmentor_builds_with_a_gn_head():
    import ddp_amd
    c = G.LOOP['b1_ddim_fused']
    model = ddp_amd.build_segmentor(dict(type='DDP', timesteps=c['K'], bit_scale=0.01, accumulation=True,
                                         decode_head=dict(type='FCNHeadWithTime', num_convs=2, concat_input=False, in_channels=256, channels=256,
                                                          num_classes=c['classes'], in_index=0, norm_cfg=dict(type='GN', num_groups=32))))
    model.load_state_dict(G.loop_state(c), strict=True)


# ---- the C ABI did not move ----------------------------------------------------------------------------------------------------
def test_abi_version_exports_and_workspace_bytes_are_the_parents():
    lib = _lib.load()
    assert _lib.ABI_VERSION == 7 and lib.ddp_abi_version() == 7
    from support import dynamic_symbols as _dynamic_symbols
    assert _dynamic_symbols(_lib.lib_path()) == sorted(_lib.EXPORTS) and len(_lib.EXPORTS) == 36
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'fcn_gn', 'parent_workspace_bytes.json')))
    got = G.workspace_bytes(lib)
    assert len(want) == 2 * len(G.HEAD) + 4 * len(G.LOOP) and got == want


def test_gn_scratch_fits_the_region_it_borrows():
    """FcnLayout::a_sb holds Mp * 256 * 6 bytes (Mp = tokens rounded up to 256); the GroupNorm scratch is the partial sums - 16 B per
    token on the fused route, 512 B per started 256-token chunk of a map otherwise - in its first 512 Mp bytes, then 256 B of
    statistics per map"""
    for c in list(G.HEAD.values()) + [dict(c, maps=c['B'] * c['r']) for c in G.LOOP.values()]:
        N = c['h'] * c['w']
        M = c['maps'] * N
        Mp = (M + 255) // 256 * 256
        partial = 16 * M if N % 32 == 0 else c['maps'] * ((N + 255) // 256) * 512
        assert partial <= 512 * Mp and 512 * Mp + 256 * c['maps'] <= 1536 * Mp


# ---- the new kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_gn_film_relu_kernel_resources(tmp_path):
    """k_gn_film_relu_blk for gfx950: no scratch, LDS = the (a | b) vectors of two maps (4 KiB), 16-byte global loads and stores and
    16-byte LDS reads only.  Registers as found when the kernel was written: 75 (asserted with room: at most 128 = 4 waves per SIMD)."""
    out = tmp_path / 'fcn_gn.s'
    src = os.path.join(ROOT, 'ddp_amd', 'csrc', 'ddp_fcn_gn.hip')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-x', 'hip', src,
                    '--cuda-device-only', '-S', '-o', str(out)], check=True, capture_output=True, timeout=600)
    text = out.read_text()
    found = re.findall(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', text, re.S)
    assert len(found) == 1 and 'k_gn_film_relu_blk' in found[0][0]
    body = found[0][1]
    vgpr = int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1))
    lds = int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1))
    print(f'k_gn_film_relu_blk: {vgpr} registers, {lds} B LDS')
    assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0
    assert lds == 2 * 2 * 256 * 4 and vgpr <= 128
    assert len(re.findall(r'global_load_dwordx4', text)) >= 8 and len(re.findall(r'global_store_dwordx4', text)) >= 8
    assert not re.findall(r'global_store_dword\s', text)          # every activation store is 16 bytes wide


# ---- drop-in, inside the reference's registry ----------------------------------------------------------------------------------
@pytest.mark.skipif(not ref_shim.available(), reason='reference tree not present (build container only)')
def test_reference_gn_head_state_dict_loads_strictly_into_ours():
    """a subprocess (the reference import mutates sys.modules / the mmcv registries): the reference's own FCNHeadWithTime with GN(32)
    gives a state_dict; after register_into_mmseg() the reference's registry builds ddp_amd's class from the same config, which loads
    that state_dict strictly, key -> shape equal"""
    code = (
        "import sys, json\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import ref_shim\n"
        "ref_shim.import_seg()\n"
        "from mmseg.models.decode_heads import FCNHeadWithTime as Ref\n"
        "from mmseg.models.builder import HEADS\n"
        "cfg = dict(type='FCNHeadWithTime', num_convs=2, kernel_size=3, concat_input=True, dilation=1, in_channels=256, channels=256,\n"
        "           num_classes=19, in_index=0, dropout_ratio=0.1, norm_cfg=dict(type='GN', num_groups=32), align_corners=False)\n"
        "ref = HEADS.build(dict(cfg))\n"
        "assert type(ref) is Ref\n"
        "import ddp_amd\n"
        "ddp_amd.register_into_mmseg()\n"
        "ours = HEADS.build(dict(cfg))\n"
        "assert type(ours) is ddp_amd.FCNHeadWithTime, type(ours)\n"
        "res = ours.load_state_dict(ref.state_dict(), strict=True)\n"
        "a = {k: tuple(v.shape) for k, v in ref.state_dict().items()}\n"
        "b = {k: tuple(v.shape) for k, v in ours.state_dict().items()}\n"
        "print(json.dumps(dict(equal=a == b, keys=len(a), gn=sorted(k for k in a if '.gn.' in k), res=str(res))))\n"
        % (ROOT, os.path.join(ROOT, 'tests', 'golden')))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert d['equal'] and 'All keys matched' in d['res']
    assert d['gn'] == ['conv_cat.gn.bias', 'conv_cat.gn.weight', 'convs.0.gn.bias', 'convs.0.gn.weight', 'convs.1.gn.bias', 'convs.1.gn.weight']
