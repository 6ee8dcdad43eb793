"""DDP_FLAG_STEP_RECORD on the CPU: what validate() accepts, and what the flag does to the workspace queries.

The flag carves two buffers at the END of the workspace (include/ddp_mi355x.h, at ddp_x0_trace): the per-step record and the
step-disagreement map, each rounded up to the carve granularity of 256 bytes.  Everything else - the model region, every offset
in front of the two buffers and the sizes of a cfg without the flag - must be what it was before the flag existed:
tests/golden/step_record/parent_workspace_bytes.json holds ddp_query_workspace / ddp_query_const_workspace (and
ddp_sample_fcn_workspace) of every case of tests/config_space_cases.py under five engine / flag variants, recorded from the
library of the commit before this feature."""
import ctypes as C
import json
import os

import pytest

import config_space_cases as S
from ddp_amd import _lib
from ddp_amd.engine import step_record_sizes
from support import lib, round256  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'step_record', 'parent_workspace_bytes.json')
VARIANTS = {'bf16x3': ('bf16x3', {}), 'f32': ('f32', {}), 'unfused-layer': ('bf16x3', dict(fused_layer=False)),
            'unfused-tail': ('bf16x3', dict(fused_tail=False)), 'unfused-prologue': ('bf16x3', dict(fused_prologue=False))}
FCN_HEADS = ((0, 1), (2, 1), (1, 2))            # (num_convs, dilation)


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def with_flags(cfg, extra):
    cfg.flags |= extra
    return cfg


def header_bytes(cfg):
    """the header's two formulas, written out here independently of the binding's helper"""
    n = cfg.batch * cfg.head_h * cfg.head_w
    return cfg.timesteps * cfg.randsteps * n * (1 if cfg.task == _lib.TASK_SEG else 4), n * 4


def test_flag_value_and_binding_formulas():
    assert _lib.FLAG_STEP_RECORD == 1024
    for name in ('seg_L12', 'depth_9x11_L2_r2', 'bev_kc9_r2', 'bev_kc5_small_grid'):
        cfg = S.make_cfg(S.CASES[name])
        assert step_record_sizes(cfg) == header_bytes(cfg)


@pytest.mark.parametrize('name', ['seg_L12', 'seg_ddpm_acc', 'depth_9x11_L2_r2', 'depth_1x37_L2_bins', 'bev_kc8_r1', 'bev_kc9_r2'])
@pytest.mark.parametrize('vid', sorted(VARIANTS))
def test_validate_accepts_the_flag_on_every_task_sampler_and_engine(lib, name, vid):
    gemm, fl = VARIANTS[vid]
    rc, total, const = S.query(lib, with_flags(S.make_cfg(S.CASES[name], gemm, **fl), _lib.FLAG_STEP_RECORD))
    assert rc == 0, lib.ddp_last_error()
    assert total > const > 0


def test_other_flags_combine_with_it(lib):
    c = S.CASES['seg_L12']
    for extra in (_lib.FLAG_RECORD_X0, _lib.FLAG_GATHER_GUESS_ZERO, _lib.FLAG_SB_HEAD, _lib.FLAG_UNFUSED_TAIL):
        assert S.query(lib, with_flags(S.make_cfg(c), _lib.FLAG_STEP_RECORD | extra))[0] == 0, lib.ddp_last_error()
    d = S.CASES['depth_9x11_L1_scale_up_no_eps']
    assert S.query(lib, with_flags(S.make_cfg(d), _lib.FLAG_STEP_RECORD))[0] == 0, lib.ddp_last_error()


def test_refused_with_force_x0(lib):
    cfg = with_flags(S.make_cfg(S.CASES['seg_L12']), _lib.FLAG_STEP_RECORD | _lib.FLAG_FORCE_X0)
    assert S.query(lib, cfg)[0] == -1
    assert b'FORCE_X0' in lib.ddp_last_error()
    # (FORCE_X0 alone is still a valid seg cfg, RECORD_X0 / FORCE_X0 are still refused outside seg)
    assert S.query(lib, with_flags(S.make_cfg(S.CASES['seg_L12']), _lib.FLAG_FORCE_X0))[0] == 0
    assert S.query(lib, with_flags(S.make_cfg(S.CASES['depth_K1']), _lib.FLAG_RECORD_X0))[0] == -1


@pytest.mark.parametrize('vid', sorted(VARIANTS))
def test_workspace_grows_by_the_two_header_formulas(lib, vid):
    """every case of the configuration sweep (task, B, r, K, map and head grid, classes, layers, feature width) x five variants:
    query(flag) - query(no flag) = round256(record_bytes) + round256(map_bytes); the model region does not move"""
    gemm, fl = VARIANTS[vid]
    for name, c in S.CASES.items():
        rc0, tot0, const0 = S.query(lib, S.make_cfg(c, gemm, **fl))
        cfg = with_flags(S.make_cfg(c, gemm, **fl), _lib.FLAG_STEP_RECORD)
        rc1, tot1, const1 = S.query(lib, cfg)
        assert rc0 == 0 and rc1 == 0, (name, lib.ddp_last_error())
        rec, smap = header_bytes(cfg)
        assert tot1 - tot0 == round256(rec) + round256(smap), (name, vid, tot1 - tot0, rec, smap)
        assert const1 == const0, (name, vid)


def test_geometry_grid_beyond_the_sweep(lib):
    """B x r x K x map sizes the sweep does not hold, incl. the issue's maps (7 x 13, 5 x 9, 1 x 37) and sizes whose record is
    (not) a multiple of 256 bytes"""
    for task, base in (('seg', 'seg_L12'), ('depth', 'depth_K1'), ('bev', 'bev_kc5_th0.3')):
        for B in (1, 2, 5):
            for r in (1, 2, 3):
                for K in (1, 3, 4, 64):
                    for h, w in ((7, 13), (5, 9), (1, 37), (1, 1), (16, 16), (33, 31)):
                        c = dict(S.CASES[base], B=B, r=r, K=K, h=h, w=w, L=2)
                        tot0 = S.query(lib, S.make_cfg(c))[1]
                        cfg = with_flags(S.make_cfg(c), _lib.FLAG_STEP_RECORD)
                        rc, tot1, _ = S.query(lib, cfg)
                        assert rc == 0, lib.ddp_last_error()
                        rec, smap = header_bytes(cfg)
                        assert rec == K * B * r * cfg.head_h * cfg.head_w * (1 if task == 'seg' else 4)
                        assert tot1 - tot0 == round256(rec) + round256(smap), (task, B, r, K, h, w)


def test_record_x0_and_step_record_share_one_buffer(lib):
    """seg with both flags: the RECORD_X0 trace IS the step record - only the map is added to the RECORD_X0 cfg"""
    for name in ('seg_L12', 'seg_cx512_r2_5x10', 'seg_ddpm_acc'):
        c = S.CASES[name]
        t_x0 = S.query(lib, with_flags(S.make_cfg(c), _lib.FLAG_RECORD_X0))[1]
        t_rec = S.query(lib, with_flags(S.make_cfg(c), _lib.FLAG_STEP_RECORD))[1]
        cfg = with_flags(S.make_cfg(c), _lib.FLAG_STEP_RECORD | _lib.FLAG_RECORD_X0)
        t_both = S.query(lib, cfg)[1]
        assert t_both == t_rec
        assert t_both - t_x0 == round256(header_bytes(cfg)[1])


def test_sizes_without_the_flag_are_the_parents(lib, golden):
    """ddp_query_workspace / ddp_query_const_workspace with the flag clear against the values recorded from the parent commit's
    library, and the model region with the flag SET against the same record"""
    seen = 0
    for name, c in S.CASES.items():
        for vid, (gemm, fl) in VARIANTS.items():
            want = golden['sample'][f'{name}/{vid}']
            rc, tot, const = S.query(lib, S.make_cfg(c, gemm, **fl))
            assert rc == 0 and [tot, const] == want, (name, vid, tot, const, want)
            assert S.query(lib, with_flags(S.make_cfg(c, gemm, **fl), _lib.FLAG_STEP_RECORD))[2] == want[1]
            seen += 1
    assert seen == len(golden['sample']) == 5 * len(S.CASES)


def _fcn_bytes(lib, cfg, num_convs, dilation):
    n = C.c_size_t(0)
    assert lib.ddp_sample_fcn_workspace(C.byref(cfg), num_convs, dilation, C.byref(n)) == 0, lib.ddp_last_error()
    return n.value


def test_fcn_loop_workspace(lib, golden):
    seen = 0
    for name, c in S.CASES.items():
        if c['task'] != 'seg':
            continue
        for nc, dil in FCN_HEADS:
            base = _fcn_bytes(lib, S.make_cfg(c), nc, dil)
            assert base == golden['fcn'][f'{name}/{nc}/{dil}']
            cfg = with_flags(S.make_cfg(c), _lib.FLAG_STEP_RECORD)
            rec, smap = header_bytes(cfg)
            assert _fcn_bytes(lib, cfg, nc, dil) - base == round256(rec) + round256(smap)
            seen += 1
    assert seen == len(golden['fcn'])
    cfg = with_flags(S.make_cfg(S.CASES['seg_L12']), _lib.FLAG_STEP_RECORD | _lib.FLAG_FORCE_X0)
    n = C.c_size_t(0)
    assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 2, 1, C.byref(n)) == -1


def test_new_translation_unit_is_built_and_hashed():
    from ddp_amd import build
    assert 'ddp_step_record.hip' in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, 'ddp_step_record.hip'))
