"""The BEV head's ``seg_conv_kernel`` and ``grid_transform.prescale_factor`` without a GPU: the CPU restatement of both operators
against the fixtures the reference made (tests/golden/bev_head/), the drop-in's constructor surface and state_dict layout, the
C ABI's validation of the two new ``ddp_cfg`` fields, the workspace sizes of configurations that set neither, and the compile-time
resources of the two new kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

import ddp_amd  # noqa: F401  (registers the drop-in classes)
from ddp_amd import _lib
from ddp_amd.bev.ddp import DDP as BEVDDP, BEVDeformableHeadWithTime
from ddp_amd.utils import synthetic
import bev_head_util as U
from golden_util import max_rel
from oracle import ddp_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
BEV_BOUND = 2e-5        # the bound tests/test_oracle_golden.py holds the BEV oracle to


# ---- restatement against the reference-made fixtures ----------------------------------------------------------------------------
@pytest.mark.parametrize('name', U.sampler_cases())
def test_cpu_restatement_matches_reference_fixture(name):
    cfg, sd, x, noise, g = U.load(name)
    assert float(g['thr_margin']) >= 1e-3          # the generator's condition: no probability next to the threshold
    trace = []
    with torch.no_grad():
        out, steps = U.sample(x, noise, sd, cfg, trace)
    assert out.shape == g['out'].shape and steps.shape == g['prob_steps'].shape
    e_out, e_steps = max_rel(out, g['out']), max_rel(steps, g['prob_steps'])
    print(f'BEV-HEAD restatement {name}: out {e_out:.3e} steps {e_steps:.3e} (bound {BEV_BOUND:.0e})')
    assert e_out <= BEV_BOUND and e_steps <= BEV_BOUND
    # same decisions at every step, every pixel
    for s, t in enumerate(trace):
        assert torch.equal(t['pred'], g['prob_steps'][s] > cfg.get('threshold', 0.5))


def test_cpu_restatement_matches_reference_head_forward():
    cfg, sd, feat, _, g = U.load('head_forward')
    with torch.no_grad():
        out = U.head_forward(feat, g['temb'], sd, cfg)
    assert out.shape == g['out'].shape
    assert max_rel(out, g['out']) <= BEV_BOUND


@pytest.mark.parametrize('p,h,w', [(2, 16, 16), (0.5, 16, 16), (1.5, 13, 9), (3, 5, 7), (0.3, 11, 4), (1.7, 1, 9)])
def test_prescale_restatement_is_f_interpolate(p, h, w):
    """the index arithmetic the kernel restates: floor(in p) outputs, source coordinate from the GIVEN factor, clamps"""
    import torch.nn.functional as F
    x = torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(5))
    want = F.interpolate(x, scale_factor=p, mode='bilinear', align_corners=False)
    got = U.prescale(x, p)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 4e-6


# ---- public interface -----------------------------------------------------------------------------------------------------------
def _head(**over):
    cfg = dict(num_layers=2, input_scope=[[-51.2, 51.2, 6.4]] * 2, output_scope=[[-50, 50, 5.0]] * 2)
    cfg.update(over)
    return BEVDeformableHeadWithTime(**U.head_kwargs(cfg)), cfg


def test_head_builds_with_both_arguments_and_loads_reference_shaped_state():
    head, cfg = _head(seg_conv_kernel=3, prescale_factor=2)
    assert tuple(head.conv_seg.weight.shape) == (6, 256, 3, 3) and tuple(head.conv_seg.bias.shape) == (6,)
    assert head.conv_seg.padding == (1, 1)
    kw = head._engine_kwargs()
    assert kw['bev_seg_kernel'] == 3 and kw['bev_prescale'] == 2.0
    sd = synthetic.make_state_dict('bev', 6, 2, 256, seed=7, seg_conv_kernel=3)
    hsd = {k[len('decode_head.'):]: v for k, v in sd.items() if k.startswith('decode_head.')}
    assert {k: tuple(v.shape) for k, v in head.state_dict().items()} == {k: tuple(v.shape) for k, v in hsd.items()}
    head.load_state_dict(hsd, strict=True)
    other, _ = _head(seg_conv_kernel=3)
    other.load_state_dict(head.state_dict(), strict=True)           # ... and back
    assert torch.equal(other.conv_seg.weight, hsd['conv_seg.weight'])
    # a 1x1 head refuses the 3x3 tensor and the other way round
    plain, _ = _head()
    assert tuple(plain.conv_seg.weight.shape) == (6, 256, 1, 1) and plain._engine_kwargs()['bev_seg_kernel'] == 1
    assert plain._engine_kwargs()['bev_prescale'] == 1.0
    with pytest.raises(RuntimeError, match='size mismatch'):
        plain.load_state_dict(hsd, strict=True)
    # the sampler's own parameters are untouched by either argument
    model = BEVDDP(timesteps=3, randsteps=1, feat_channels=256)
    model.load_state_dict({k: v for k, v in sd.items() if not k.startswith('decode_head.')}, strict=True)


def test_other_kernel_sizes_and_bad_factors_raise():
    """(the reference builds a 3x3 conv_seg for ANY seg_conv_kernel other than 1; here only 1 and 3 are accepted)"""
    for k in (2, 5, 0):
        with pytest.raises(ValueError, match='seg_conv_kernel'):
            _head(seg_conv_kernel=k)
    for p in (0, -1.0, float('inf')):
        with pytest.raises(ValueError, match='prescale_factor'):
            _head(prescale_factor=p)
    from ddp_amd.engine import check_bev_head
    with pytest.raises(ValueError, match='empty'):
        check_bev_head(0.3, 1, 3, 16)                # floor(3 * 0.3) = 0
    assert check_bev_head(1.5, 3, 13, 9) == (1.5, 3)


@pytest.mark.parametrize('p', [0.9, 0.7, 1.4, 0.3, 1.7, 1.1, 0.6, 2.3, 0.5, 1.5, 2, 3])
def test_factor_handed_to_the_library_gives_the_reference_sizes(p):
    """The ABI field is a float and the library sizes the prescaled map as floor(in * double(float p)); F.interpolate uses the Python
    double.  float32(0.9) gives 8 columns of a 10-wide map, the reference 9: check_bev_head hands over the neighbouring float that
    gives the reference's sizes (or raises), for every map size up to 256."""
    import math
    import numpy as np
    import torch.nn.functional as F
    from ddp_amd.engine import check_bev_head
    moved = 0
    for n in range(1, 257):
        if math.floor(n * p) < 1:
            continue
        q, _ = check_bev_head(p, 1, n, n)
        assert float(np.float32(q)) == q and abs(q - p) <= 2.0 ** -22 * p
        want = F.interpolate(torch.zeros(1, 1, n, 1), scale_factor=(p, 1), mode='bilinear', align_corners=False).shape[2]
        assert math.floor(n * float(C.c_float(q).value)) == want == math.floor(n * p), (p, n)
        moved += q != float(np.float32(p))
    if p in (0.9, 0.7):
        assert moved > 0            # (the cases named in the header: float32(p) itself falls one short somewhere)
    # both axes at once
    q, _ = check_bev_head(0.9, 1, 12, 10)
    assert (math.floor(12 * q), math.floor(10 * q)) == (10, 9)


def test_synthetic_default_is_unchanged_and_kernel_3_is_3x3():
    a = synthetic.make_state_dict('bev', 6, 2, 256, seed=11)
    b = synthetic.make_state_dict('bev', 6, 2, 256, seed=11, seg_conv_kernel=1)
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
    assert tuple(a['decode_head.conv_seg.weight'].shape) == (6, 256, 1, 1)
    # pinned: the default's tensors are the ones the committed 1x1 fixtures were made from
    import numpy as np
    z = np.load(os.path.join(HERE, 'golden', 'bev_fusion.npz'))
    sd = synthetic.make_state_dict('bev', 6, 5, 512, seed=20 + 100)
    assert abs(synthetic.checksum(sd) - float(z['weights_fp'])) <= 1e-9 * abs(float(z['weights_fp']))
    c = synthetic.make_state_dict('bev', 6, 2, 256, seed=11, seg_conv_kernel=3)
    assert tuple(c['decode_head.conv_seg.weight'].shape) == (6, 256, 3, 3)
    for k in a:                                      # everything drawn before conv_seg is the same
        if 'conv_seg' not in k:
            assert torch.equal(a[k], c[k]), k
    with pytest.raises(ValueError):
        synthetic.make_state_dict('seg', 6, 2, 256, seed=11, seg_conv_kernel=3)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def _cfg(task=_lib.TASK_BEV, **kw):
    c = _lib.DdpCfg()
    c.abi_version = _lib.ABI_VERSION
    c.task = task
    c.batch, c.randsteps, c.timesteps, c.num_layers = 1, 1, 3, 4
    c.num_classes = 1 if task == _lib.TASK_DEPTH else 6
    c.feat_channels = 256
    c.h, c.w = 16, 16
    c.head_h, c.head_w = (20, 20) if task == _lib.TASK_BEV else (16, 16)
    c.bit_scale, c.min_depth, c.max_depth, c.threshold = 0.01, 1e-3, 80.0, 0.5
    for a in range(2):
        c.bev_in_min[a], c.bev_in_max[a], c.bev_out_first[a], c.bev_out_step[a] = -51.2, 51.2, -47.5, 5.0
    c.gemm_mode = _lib.GEMM_BF16X3
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _query(cfg, const=False):
    lib = _lib.load()
    n = C.c_size_t(0)
    fn = lib.ddp_query_const_workspace if const else lib.ddp_query_workspace
    rc = fn(C.byref(cfg), C.byref(n))
    return rc, n.value, lib.ddp_last_error().decode()


def test_abi_is_7_with_two_appended_fields_and_36_exports():
    assert _lib.ABI_VERSION == 7 and _lib.load().ddp_abi_version() == 7
    names = [f[0] for f in _lib.DdpCfg._fields_]
    assert names[-2:] == ['bev_prescale', 'bev_seg_kernel'] and names[-3] == 'head_max_depth'
    assert C.sizeof(_lib.DdpCfg) == 34 * 4
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'ddp_mi355x.h')).read()
    assert '#define DDP_ABI_VERSION 7' in header and '#define DDP_BEV_MAX_PRESCALE_AREA 16' in header
    assert len(_lib.EXPORTS) == 36 and len(set(_lib.EXPORTS)) == 36
    nm = shutil.which('nm')
    if nm:
        out = subprocess.run([nm, '-D', '--defined-only', _lib.lib_path()], capture_output=True, text=True, check=True).stdout
        syms = sorted(l.split()[-1] for l in out.splitlines() if ' T ' in l)
        assert syms == sorted(_lib.EXPORTS), syms


@pytest.mark.parametrize('kernel', [2, 5, -3, 4])
def test_validate_refuses_other_kernel_sizes(kernel):
    rc, _, err = _query(_cfg(bev_seg_kernel=kernel))
    assert rc == -1 and 'bev_seg_kernel' in err


@pytest.mark.parametrize('task', [_lib.TASK_SEG, _lib.TASK_DEPTH])
@pytest.mark.parametrize('field,value', [('bev_seg_kernel', 3), ('bev_seg_kernel', 1), ('bev_prescale', 2.0), ('bev_prescale', 1.0)])
def test_validate_refuses_a_non_bev_task_with_a_field_set(task, field, value):
    rc, _, err = _query(_cfg(task=task))
    assert rc == 0, err
    rc, _, err = _query(_cfg(task=task, **{field: value}))
    assert rc == -1 and 'bev head only' in err


def test_validate_refuses_empty_and_oversized_prescaled_maps():
    rc, _, err = _query(_cfg(h=3, w=16, bev_prescale=0.3))            # floor(3 * 0.3) = 0
    assert rc == -1 and 'empty' in err
    rc, _, err = _query(_cfg(h=16, w=1, bev_prescale=0.5))            # floor(1 * 0.5) = 0
    assert rc == -1 and 'empty' in err
    rc, _, err = _query(_cfg(bev_prescale=-2.0))
    assert rc == -1 and 'bev_prescale' in err
    rc, _, err = _query(_cfg(bev_prescale=float('nan')))
    assert rc == -1 and 'bev_prescale' in err
    # the bound of the header: the prescaled map may have up to DDP_BEV_MAX_PRESCALE_AREA times the pixels of the map
    rc, n4, err = _query(_cfg(bev_prescale=4.0))
    assert rc == 0, err
    rc, _, err = _query(_cfg(bev_prescale=4.25))                      # 68 x 68 > 16 * 16 * 16
    assert rc == -1 and 'exceeds' in err
    # the buffer is accounted for: B r maps of (hp, wp) x 256 floats
    rc, n1, _ = _query(_cfg())
    assert n4 - n1 >= 64 * 64 * 256 * 4
    rc, n2, _ = _query(_cfg(bev_prescale=2.0, batch=2, randsteps=3))
    rc, n0, _ = _query(_cfg(batch=2, randsteps=3))
    assert n2 - n0 >= 6 * 32 * 32 * 256 * 4
    # valid values pass on both engines, together and alone
    for gm in (_lib.GEMM_BF16X3, _lib.GEMM_F32_MFMA):
        for kw in (dict(bev_seg_kernel=3), dict(bev_prescale=0.5), dict(bev_prescale=1.5, bev_seg_kernel=3, h=13, w=9)):
            rc, _, err = _query(_cfg(gemm_mode=gm, **kw))
            assert rc == 0, err


# ddp_query_workspace / ddp_query_const_workspace of the ABI-6 library (the parent commit's build, queried with its own 32-word
# ddp_cfg) on the grid below: (total, const) bytes.  A configuration that sets neither new field must keep them.
_GRID = [dict(batch=b, randsteps=r, num_classes=k, feat_channels=cx, h=h, w=w, head_h=hh, head_w=wh, num_layers=L, gemm_mode=gm, flags=fl)
         for (b, r, k, cx, h, w, hh, wh, L) in [(1, 1, 6, 256, 16, 16, 20, 20, 4), (2, 4, 6, 512, 16, 16, 20, 20, 5),
                                                 (1, 2, 1, 256, 13, 9, 25, 16, 2), (1, 1, 8, 96, 5, 7, 1, 9, 1),
                                                 (2, 1, 9, 256, 14, 10, 25, 16, 3), (1, 1, 32, 256, 7, 7, 10, 10, 2),
                                                 (8, 1, 6, 512, 200, 200, 200, 200, 6)]
         for gm in (_lib.GEMM_BF16X3, _lib.GEMM_F32_MFMA)
         for fl in ((0, _lib.FLAG_UNFUSED_TAIL, _lib.FLAG_UNFUSED_LAYER) if gm == _lib.GEMM_BF16X3 else (0,))]
_ABI6_SIZES = [
    (51457024, 39577600), (51457024, 39577600), (51457024, 39577600), (6078976, 1010176),
    (127236096, 48508928), (127236096, 48508928), (127236096, 48508928), (35227648, 1383424),
    (45567488, 22885888), (45567488, 22885888), (45567488, 22885888), (9866752, 782848),
    (19734528, 14738432), (19734528, 14738432), (19734528, 14738432), (2319360, 515072),
    (54232064, 31178240), (54232064, 31178240), (54232064, 31178240), (10358272, 902144),
    (28356096, 22961152), (28356096, 22961152), (28356096, 22961152), (2903040, 814592),
    (8625140736, 56784896), (8625140736, 56784896), (8625140736, 56784896), (3811696128, 1494528)
]


def test_workspace_of_zeroed_fields_equals_the_abi6_sizes():
    assert len(_GRID) == len(_ABI6_SIZES) == 28
    for kw, (total6, const6) in zip(_GRID, _ABI6_SIZES):
        got = {}
        for k in (0, 1):
            for p in (0.0, 1.0):
                rc, n, err = _query(_cfg(bev_seg_kernel=k, bev_prescale=p, **kw))
                assert rc == 0, err
                rc, nc, err = _query(_cfg(bev_seg_kernel=k, bev_prescale=p, **kw), const=True)
                assert rc == 0, err
                got[(k, p)] = (n, nc)
        assert set(got.values()) == {(total6, const6)}, (kw, got, (total6, const6))
        # (and the variants do cost something: the test would not notice a carve() that ignores the fields)
        assert _query(_cfg(bev_seg_kernel=3, **kw))[1] > total6 and _query(_cfg(bev_prescale=2.0, **kw))[1] > total6


# ---- kernels --------------------------------------------------------------------------------------------------------------------
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_new_kernels_have_no_scratch(tmp_path):
    """k_bev_seg3 keeps a token's <= 8 logit quads in registers, k_bev_prescale four corner rows: byte-streaming kernels, a spill
    would be vector memory in the middle of the stream (read as tests/test_kernel_resources.py reads it)"""
    out = tmp_path / 'kernels.s'
    src = os.path.join(os.path.dirname(HERE), 'ddp_amd', 'csrc', 'ddp_kernels.hip')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-x', 'hip', src,
                    '--cuda-device-only', '-S', '-o', str(out)], check=True, capture_output=True, timeout=600)
    found = set()
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', out.read_text(), re.S):
        for k in ('k_bev_seg3', 'k_bev_prescale'):
            if k in m.group(1):
                found.add(k)
                body = m.group(2)
                assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, m.group(1)
                assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 128, m.group(1)
    assert found == {'k_bev_seg3', 'k_bev_prescale'}
