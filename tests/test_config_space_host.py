"""CPU companion of tests/test_config_space_gpu.py: for every case of tests/config_space_cases.py the host entries of the C ABI
accept the configuration, every refusal the sweep names comes back as DDP_E_BADCFG with a message, and the oracle the GPU test
compares with is well conditioned on the case (fp32 within REL / 20 of its own fp64 evaluation - the condition under which the
existing bar REL applies to the case unchanged).  No GPU compute is invoked."""
import ctypes as C

import pytest
import torch

import config_space_cases as S
from ddp_amd import _lib
from golden_util import max_rel


def _rp(rows):
    """rows of an operand of the bf16x3 GEMMs: staged in whole 64-row blocks, read in whole 256-row tiles"""
    return (rows + 255) // 256 * 256


@pytest.mark.parametrize('name', S.names())
def test_workspace_queries_accept_every_case(name):
    """ddp_query_workspace succeeds for the case on both engines and under every diagnostic flag; the model region
    (ddp_query_const_workspace) does not depend on batch, randsteps or the map size; the workspace holds at least the buffers
    whose sizes follow from the header's tensor shapes (a lower bound made here, independent of carve())."""
    lib = _lib.load()
    c = S.CASES[name]
    for gemm in ('bf16x3', 'f32'):
        for flags in ({}, dict(fused_tail=False), dict(fused_layer=False), dict(fused_prologue=False), dict(nchw_head=False)):
            rc, total, model = S.query(lib, S.make_cfg(c, gemm, **flags))
            assert rc == 0, lib.ddp_last_error()
            assert 0 < model < total and total % 256 == 0
            for geo in (dict(B=c['B'] + 3), dict(r=c['r'] + 1), dict(h=c['h'] + 5, w=c['w'] + 2), dict(B=1, r=1, h=1, w=1)):
                rc2, total2, model2 = S.query(lib, S.make_cfg(dict(c, **geo), gemm, **flags))
                assert rc2 == 0 and model2 == model, (geo, model, model2)
            # what any implementation must hold at once: x as the operand of the x projection (bf16x3: whole 256-row tiles of B.N
            # rows x Cx values, three bf16 pieces each = 6 bytes; fp32 engine: B.N.Cx floats), its result (B.N.256), the FFN hidden
            # layer of all tokens (M.1024) and q (M.256)
            hh, wh = S.head_grid(c)
            bn, m = c['B'] * c['h'] * c['w'], c['B'] * c['r'] * hh * wh
            floor = (_rp(bn) * c['Cx'] * 6 if gemm == 'bf16x3' else bn * c['Cx'] * 4) + 4 * (bn * 256 + m * 256) + 4 * m * 1024
            assert total - model >= floor, (total - model, floor)


@pytest.mark.parametrize('task', ['seg', 'depth', 'bev'])
@pytest.mark.parametrize('bn,r,cx', [(100, 2, 512), (65, 3, 768), (66, 3, 768), (10, 2, 512), (100, 3, 736), (130, 2, 512), (252, 2, 512),
                                      (200, 4, 1024), (31, 8, 2048), (100, 1, 512), (100, 2, 256), (300, 2, 1056)])
def test_workspace_covers_the_padded_x_operand(task, bn, r, cx):
    """The guard check of the GPU sweep, validated on the CPU: the sum the workspace must reach, against ddp_query_workspace.
    On the bf16x3 engine one staging buffer serves the noisy map / layer input (r.B.N rows of 256 channels) and x (B.N rows of Cx),
    each in whole 256-row tiles of 6-byte elements.  Everything else of the geometry region is independent of Cx or grows with
    it, so against the same geometry at Cx = 32 (where the noisy map decides) the region must grow by at least what x needs beyond
    the noisy map's buffer.  (100, 2, 512) and (65, 3, 768) are the points where a comparison of the UNPADDED products picked the
    smaller buffer: 384 KiB read, 192 KiB written past the end of the workspace."""
    lib = _lib.load()
    c = dict(S.CASES[{'seg': 'seg_cx512_r2', 'depth': 'depth_cx512', 'bev': 'bev_cx1056'}[task]], B=1, h=1, w=bn, r=r)
    if task == 'bev':
        c['grid'] = (0, 0)
    rc0, t0, m0 = S.query(lib, S.make_cfg(dict(c, Cx=32)))
    rc1, t1, m1 = S.query(lib, S.make_cfg(dict(c, Cx=cx)))
    assert rc0 == 0 and rc1 == 0
    hh, wh = S.head_grid(c)
    rows = max(r * bn, r * hh * wh)
    need_more = max(0, _rp(bn) * cx * 6 - _rp(rows) * 256 * 6)
    assert (t1 - m1) - (t0 - m0) >= need_more, ((t1 - m1) - (t0 - m0), need_more)


@pytest.mark.parametrize('base,over,word', S.REFUSALS)
def test_limits_are_refused_with_a_message(base, over, word):
    """one past every limit validate() states (32 BEV classes, DDP_MAX_LAYERS, DDP_MAX_STEPS): DDP_E_BADCFG and a message that
    names the field, from both query entries; the limit itself is accepted"""
    lib = _lib.load()
    c = S.CASES[base]
    assert S.query(lib, S.make_cfg(c))[0] == 0
    cfg = S.make_cfg(dict(c, **over))
    n = C.c_size_t(0)
    for entry in (lib.ddp_query_workspace, lib.ddp_query_const_workspace):
        assert entry(C.byref(cfg), C.byref(n)) == -1          # DDP_E_BADCFG
        assert word.encode() in lib.ddp_last_error(), lib.ddp_last_error()


def test_every_family_has_its_members():
    """the sweep the GPU test runs: the members each family must have (a case dropped from the list fails here, on the CPU)"""
    have = set(S.names())
    want = {f'bev_kc{k}_r{r}' for k in (1, 2, 3, 7, 8, 9, 16, 31, 32) for r in (1, 2)}
    want |= {f'seg_cx{cx}_r{r}' for cx in (32, 96, 512, 1056, 2048) for r in (1, 2)}
    want |= {'seg_cx512_r2_5x10', 'seg_cx768_r3_3x11', 'depth_cx512_r2_5x10', 'bev_cx512_r2_5x10'}
    want |= {'depth_cx32', 'depth_cx512', 'bev_cx32', 'bev_cx1056', 'seg_L12', 'depth_L12_r2', 'bev_L12', 'seg_K64_L12', 'seg_K64_noacc',
             'depth_K64', 'depth_K1', 'bev_K1', 'seg_ddpm_acc', 'seg_ddpm_noacc', 'depth_1x37_L3', 'depth_1x1_L2', 'depth_23x1_L2',
             'depth_9x11_L1', 'depth_1x37_L2_bins', 'depth_9x11_L1_bins'}
    assert want <= have, want - have
    for c in S.CASES.values():
        hh, wh = S.head_grid(c)
        degenerate = min(c['h'], c['w']) == 1
        assert c['B'] in (2, 3) and (degenerate or ((c['h'] * c['w']) % 32 and (hh * wh) % 32)), c['name']
    thr = {c['threshold'] for c in S.CASES.values() if c['task'] == 'bev'}
    assert {0.3, 0.5, 0.7} <= thr
    grids = [(S.head_grid(c), (c['h'], c['w'])) for c in S.CASES.values() if c['task'] == 'bev']
    assert any(g[0] < m[0] and g[1] < m[1] for g, m in grids) and any(g[0] > m[0] and g[1] > m[1] for g, m in grids)


@pytest.mark.parametrize('name', S.names())
def test_oracle_is_well_conditioned_on_the_case(name):
    """fp32 oracle vs fp64 oracle on the case's own weights and inputs: max-rel < REL / 20 = 1e-5 and identical decisions
    (argmax / > threshold).  A case that misses this is replaced (another seed or size), never given a wider bar.  BEV: the
    thresholded maps are mixed (neither all-zero nor all-one codes), so the u chain's table is indexed beyond row 0."""
    c = S.CASES[name]
    r32, r64 = S.oracle_batch(c, torch.float32), S.oracle_batch(c, torch.float64)
    assert r32.dtype == torch.float32 and r64.dtype == torch.float64 and r32.shape == r64.shape
    assert torch.isfinite(r64).all()
    err = max_rel(r32.double(), r64)
    d32, d64 = S.decisions(c, r32), S.decisions(c, r64)
    agree = 1.0 if d32 is None else float((d32 == d64).float().mean())
    print(f'{name}: fp32 vs fp64 oracle max-rel {err:.2e} (cap {S.COND:.0e}), decisions equal {agree:.4f}')
    assert err < S.COND and agree > 0.9995
    if c['task'] == 'bev' and c['K'] > 1:
        above = float(d64.float().mean())
        assert 0.1 < above < 0.9, above
