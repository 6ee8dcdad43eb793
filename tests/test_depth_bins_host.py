"""Binned depth head (``classify=True``) and the split depth range, without a GPU: the drop-in's constructor surface and state_dict
layout, the bin tables, the C ABI's validation of the new ``ddp_cfg`` fields, and a CPU restatement of the binned sampler against
the fixtures the reference made (tests/golden/depth_bins/)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import ref_shim  # noqa: E402

import ddp_amd  # noqa: E402
from ddp_amd import _lib  # noqa: E402
from ddp_amd.utils import synthetic  # noqa: E402
import depth_bins_util as U  # noqa: E402
from golden_util import max_rel  # noqa: E402

KITTI = dict(min_depth=1e-3, max_depth=80, bit_scale=0.1, timesteps=3, randsteps=1)


def _build(**head):
    return ddp_amd.build_depther(U.depther_cfg(KITTI, **head)).eval()


def test_classify_depther_builds_with_the_reference_head_layout():
    m = _build(classify=True, n_bins=64, norm_strategy='softmax')
    head = m.decode_head
    assert head.classify and head.n_bins == 64 and head.bins_strategy == 'UD' and head.norm_strategy == 'softmax'
    assert tuple(head.conv_depth.weight.shape) == (64, 256, 3, 3) and tuple(head.conv_depth.bias.shape) == (64,)
    # the hot-path keys / shapes of the reference depther with the binned head (the generator loads this state_dict into the
    # reference model with every hot-path key matched)
    sd = synthetic.make_state_dict('depth', 1, 6, 256, seed=0, n_bins=64)
    ours = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert ours == {k: tuple(v.shape) for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    m2 = _build(classify=True, n_bins=64, norm_strategy='softmax')
    m2.load_state_dict(m.state_dict(), strict=True)
    assert torch.equal(m2.decode_head.conv_depth.weight, sd['decode_head.conv_depth.weight'])
    # the reference's default is 256 bins, 'UD', 'linear'
    d = _build(classify=True)
    assert d.decode_head.n_bins == 256 and d.decode_head.bins_strategy == 'UD' and d.decode_head.norm_strategy == 'linear'
    # a regression head keeps its one output channel whatever n_bins says (all DDP configs spell n_bins=None)
    r = _build(n_bins=None)
    assert tuple(r.decode_head.conv_depth.weight.shape) == (1, 256, 3, 3)


def test_bad_strategies_raise_like_the_reference():
    with pytest.raises(AssertionError, match='bins_strategy'):
        _build(classify=True, n_bins=8, bins_strategy='LID')
    with pytest.raises(AssertionError, match='norm_strategy'):
        _build(classify=True, n_bins=8, norm_strategy='tanh')
    with pytest.raises(ValueError, match='depth bins'):
        _build(classify=True, n_bins=257)


@pytest.mark.parametrize('strategy', ['UD', 'SID'])
def test_bin_tables_are_the_reference_torch_calls(strategy):
    for lo, hi, n in ((1e-3, 80.0, 256), (0.0, 1.0, 24), (1e-3, 10.0, 100)):
        m = _build(classify=True, n_bins=n, bins_strategy=strategy, min_depth=lo, max_depth=hi)
        want = torch.linspace(lo, hi, n) if strategy == 'UD' else torch.logspace(lo, hi, n)
        got = m.decode_head.depth_bins()
        assert got.dtype == torch.float32 and torch.equal(got, want)
    # SID at KITTI's range: base-10 exponents taken literally, as the reference does (inf, not rejected)
    m = _build(classify=True, n_bins=16, bins_strategy='SID')
    assert torch.isinf(m.decode_head.depth_bins()).any()


def _cfg(task=_lib.TASK_DEPTH, **kw):
    c = _lib.DdpCfg()
    c.abi_version = _lib.ABI_VERSION
    c.task = task
    c.batch, c.randsteps, c.timesteps, c.num_layers = 1, 1, 3, 6
    c.num_classes = 1 if task == _lib.TASK_DEPTH else 19
    c.feat_channels = 256
    c.h = c.head_h = 88
    c.w = c.head_w = 304
    c.bit_scale, c.min_depth, c.max_depth = 0.1, 1e-3, 80.0
    c.gemm_mode = _lib.GEMM_BF16X3
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _query(cfg):
    lib = _lib.load()
    n = C.c_size_t(0)
    rc = lib.ddp_query_workspace(C.byref(cfg), C.byref(n))
    return rc, n.value, lib.ddp_last_error().decode()


def test_workspace_query_accepts_bins_and_refuses_the_rest():
    rc0, base, _ = _query(_cfg())
    assert rc0 == 0
    sizes = {}
    for nb in (1, 100, 256):
        rc, n, err = _query(_cfg(depth_n_bins=nb, depth_norm=_lib.DEPTH_NORM_SOFTMAX))
        assert rc == 0, err
        sizes[nb] = n
    # the logits buffer: the stream GEMM's 256-channel fragment-major output, whatever n_bins is
    assert sizes[1] == sizes[256] and sizes[1] - base >= 16 * 88 * 304 * 256 * 4 // 16
    rc, _, err = _query(_cfg(depth_n_bins=257))
    assert rc < 0 and 'depth_n_bins' in err
    rc, _, err = _query(_cfg(depth_n_bins=-1))
    assert rc < 0 and 'depth_n_bins' in err
    for task in (_lib.TASK_SEG, _lib.TASK_BEV):
        rc, _, err = _query(_cfg(task=task, depth_n_bins=8, head_h=88, head_w=304))
        assert rc < 0 and 'depth' in err
    rc, _, err = _query(_cfg(depth_norm=_lib.DEPTH_NORM_SOFTMAX))          # a norm without bins
    assert rc < 0 and 'depth_norm' in err
    rc, _, err = _query(_cfg(depth_n_bins=8, depth_norm=3))
    assert rc < 0 and 'depth_norm' in err
    rc, _, err = _query(_cfg(task=_lib.TASK_SEG, head_max_depth=10.0))
    assert rc < 0 and 'head_min_depth' in err
    # the fp32 engine's buffers (zero-bordered grid + logits rows of n_bins rounded to 4) are accounted for as well
    rc, n32, err = _query(_cfg(depth_n_bins=100, gemm_mode=_lib.GEMM_F32_MFMA))
    rc0, b32, _ = _query(_cfg(gemm_mode=_lib.GEMM_F32_MFMA))
    assert rc == 0 and n32 - b32 >= 16 * 90 * 306 * (256 + 100) * 4 // 16


@pytest.mark.parametrize('name', U.sampler_cases())
def test_cpu_restatement_matches_reference_fixture(name):
    cfg, sd, x, noise, g = U.load(name)
    with torch.no_grad():
        out = U.sample(x, noise, sd, cfg)
    assert out.shape == g['out'].shape
    assert max_rel(out, g['out']) < 2e-4, name
    head = U.head_of(cfg)
    assert max_rel(out.clamp(head['min_depth'], head['max_depth']), g['out_clamped']) < 2e-4


def test_cpu_restatement_matches_reference_head_forward():
    cfg, sd, feat, _, g = U.load('head_forward')
    with torch.no_grad():
        out = U.head_forward(feat, g['temb'], sd, U.head_of(cfg))
    assert max_rel(out, g['out']) < 2e-4


_PROBE = r'''
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests', 'golden'))
import ref_shim
build_depther, Config = ref_shim.import_depth()
import ddp_amd


def model_cfg():
    m = Config.fromfile(os.path.join(ref_shim.REF, 'depth/configs/ddp_kitti/ddp_swint_1k_w7_kitti_bs2x8_scale01.py')).model
    m.backbone.init_cfg = None
    m.train_cfg = None
    m.decode_head.update(classify=True, n_bins=64, bins_strategy='SID', norm_strategy='sigmoid')
    return m


hot = lambda model: {k: v for k, v in model.state_dict().items() if not k.startswith(('backbone.', 'neck.'))}
ref = build_depther(model_cfg())
ddp_amd.register_into_mmseg()
ours = build_depther(model_cfg())
a, b = hot(ref), hot(ours)
r1 = ours.load_state_dict(a, strict=False)
r2 = ref.load_state_dict(b, strict=False)
print(json.dumps(dict(cls=type(ours).__module__ + '.' + type(ours).__name__,
                      head=type(ours.decode_head).__module__ + '.' + type(ours.decode_head).__name__,
                      n_bins=ours.decode_head.n_bins, strategy=ours.decode_head.bins_strategy, norm=ours.decode_head.norm_strategy,
                      same_shapes={k: tuple(v.shape) for k, v in a.items()} == {k: tuple(v.shape) for k, v in b.items()},
                      unexpected=list(r1.unexpected_keys) + list(r2.unexpected_keys),
                      missing_hot=[k for k in list(r1.missing_keys) + list(r2.missing_keys) if not k.startswith(('backbone.', 'neck.'))])))
'''


@pytest.mark.skipif(not ref_shim.available(), reason='reference tree not present')
def test_dropin_builds_in_the_reference_depth_registry_with_classify_kwargs():
    r = subprocess.run([sys.executable, '-c', _PROBE, os.path.dirname(HERE)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    import json
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert d['cls'] == 'ddp_amd.depther.ddp.DDP' and d['head'] == 'ddp_amd.depther.ddp.DepthDeformableHeadWithTime'
    assert (d['n_bins'], d['strategy'], d['norm']) == (64, 'SID', 'sigmoid')
    assert d['same_shapes'] and d['unexpected'] == [] and d['missing_hot'] == []


HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_depth_bins_kernel_has_no_scratch(tmp_path):
    """k_depth_bins streams a pixel's logits through three running sums: no scratch (a spill would be vector memory in the
    middle of an HBM-bound stream), one LDS table of DDP_MAX_DEPTH_BINS floats."""
    out = tmp_path / 'kernels.s'
    src = os.path.join(os.path.dirname(HERE), 'ddp_amd', 'csrc', 'ddp_kernels.hip')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-x', 'hip', src,
                    '--cuda-device-only', '-S', '-o', str(out)], check=True, capture_output=True, timeout=600)
    found = 0
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', out.read_text(), re.S):
        if 'k_depth_bins' not in m.group(1) and 'k_blk_to_pad' not in m.group(1):
            continue
        found += 1
        body = m.group(2)
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, m.group(1)
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 128, m.group(1)
    assert found == 2
