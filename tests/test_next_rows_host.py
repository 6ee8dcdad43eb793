"""CPU companion of tests/test_next_rows_gpu.py: for every case of tests/next_rows_cases.py

  * the oracle the GPU test compares with is well conditioned (fp32 within COND = REL / 20 of its own fp64 evaluation, the rule
    of tests/config_space_cases.py) - the condition under which the suite bar REL applies to the case unchanged;
  * where the GPU test compares decisions (epilogue class maps, the loop's argmax) the oracle's own near-ties (top-2 margin
    <= 1e-5) are fewer than 1e-3 of the pixels, and none at all on maps of fewer than 1000 pixels - so "no mismatch above the
    margin and fewer than 1e-3 mismatches" is an assertion the reference alone satisfies;
  * the GroupNorm-statistics route the table states for every FPN level follows from the shapes;
  * the workspace the library asks for is the sum of the buffers its layouts carve (restated here from the layout structs of
    csrc/ddp_api.hip: msm_layout, fpn_layout, their chained form, fcn_layout, fcn_loop_layout) - the GPU test then runs every
    call through a guarded workspace of exactly that size.

The library loads without a GPU; no GPU compute is invoked."""
import ctypes as C

import pytest
import torch

import next_rows_cases as N
from ddp_amd import _lib
from golden_util import max_rel
from oracle import ddp_oracle as O


def _r256(n):
    return (n + 255) // 256 * 256


_rows = _r256      # rows of a GEMM operand: whole 256-row tiles (the same rounding as the 256-byte alignment of every buffer)


def test_bar_is_the_suite_bar():
    from support import REL
    import config_space_cases as S
    assert N.REL is S.REL and N.COND is S.COND and N.REL == REL == 2e-4 and N.COND == REL / 20


# ---- the table itself -----------------------------------------------------------------------------------------------------------
def test_every_family_has_its_members():
    """the sweep the GPU test runs (a case dropped from a table fails here, on the CPU)"""
    assert set(N.NECK) >= {'all32_min', 'all32_straddle', 'mixed_low_ragged', 'one_pixel_b1', 'one_pixel_b2', 'one_row', 'one_col',
                           'flat_pyramid', 'chan_min', 'chan_max', 'swin_l', 'tiles_gt_cus', 'coarse_larger'}
    assert N.NECK['chan_min']['channels'] == [64] * 4 and N.NECK['chan_max']['channels'] == [4096, 2336, 1536, 64]
    assert sum(ch > 2304 for ch in N.NECK['chan_max']['channels']) == 2
    assert N.NECK['swin_l']['channels'] == [192, 384, 768, 1536] and N.NECK['swin_l']['levels'][3] == (16, 32)
    c = N.NECK['tiles_gt_cus']
    assert c['B'] * c['levels'][0][0] * c['levels'][0][1] // 256 > 256 and c['B'] == 2
    c = N.NECK['all32_straddle']
    assert c['B'] == 3 and all((c['B'] * h * w) % 32 == 0 and (c['B'] * h * w) % 256 for h, w in c['levels'])
    c = N.NECK['coarse_larger']
    assert c['levels'][1][0] > c['levels'][0][0]
    f = N.FCN.values()
    assert {0, 3, 8} <= {c['num_convs'] for c in f} and {1, 32, 33, 255, 256} <= {c['classes'] for c in f}
    assert {(c['dilation']) for c in f if (c['h'], c['w']) == (5, 7)} >= {1, 3, 16}
    for geo in ((1, 1, 1), (2, 1, 37), (2, 37, 1), (1, 16, 16), (1, 1, 257), (3, 10, 10)):
        assert {c['dilation'] for c in f if (c['maps'], c['h'], c['w']) == geo} >= {3, 16}, geo
    assert {(c['bn'], c['time']) for c in f} == {(True, True), (True, False), (False, True), (False, False)}
    assert len(N.FCN) <= 24
    lp = N.LOOP.values()
    assert any(c['B'] == 2 and c['r'] == 2 and c['K'] == 3 and c['sampler'] == 'ddim' and c['classes'] == 19 and (c['h'], c['w']) == (6, 9)
               for c in lp)
    assert any(c['B'] == 3 and c['r'] == 1 and c['sampler'] == 'ddpm' and c['classes'] == 150 and (c['h'], c['w']) == (5, 11) for c in lp)
    assert any(c['B'] == 2 and c['r'] == 2 and c['sampler'] == 'ddpm' for c in lp)
    assert {64, 512} <= {c['Cx'] for c in lp if c['B'] == 2} and {0, 8} <= {c['num_convs'] for c in lp}
    assert any(c['K'] == _lib.MAX_STEPS and c['num_convs'] == 1 and (c['h'], c['w']) == (3, 4) for c in lp)
    assert len(N.EPI['aug_16']['augs']) == _lib.MAX_AUGS == 16 and len(N.EPI['depth_16']['augs']) == 16
    ys, xs, crop = N.slide_grid(N.EPI['slide_64'])
    assert len(ys) == len(xs) == 8 and len(ys) * len(xs) == _lib.MAX_WINDOWS and crop == (4, 4)
    from ddp_amd.engine import slide_windows
    e = N.EPI['slide_64']
    assert slide_windows(e['img'], e['crop_size'], e['stride']) == (ys, xs, crop)      # the product cuts the same grid
    assert {c['K'] for c in N.EPI.values() if c['kind'] == 'post'} >= {1, 2, 256}


@pytest.mark.parametrize('name', N.neck_names())
def test_route_statements_follow_from_the_shapes(name):
    """'epilogue' <=> h * w % 32 == 0 (fpn_core: gn_partial of the stream GEMM), all32 <=> every level (k_gn_final32_multi)"""
    c = N.NECK[name]
    want = [N.E if (h * w) % 32 == 0 else N.S for h, w in c['levels']]
    assert c['routes'] == want, (c['routes'], want)
    assert c['all32'] == all(r == N.E for r in want)
    assert len(c['levels']) == len(c['channels']) == 4 and all(ch % 32 == 0 and 64 <= ch <= 4096 for ch in c['channels'])


def test_routes_cover_every_mix():
    mixes = {tuple(c['routes']) for c in N.NECK.values()}
    assert (N.E,) * 4 in mixes and (N.S,) * 4 in mixes
    assert any(m[0] == N.S and N.E in m for m in mixes) and any(m[0] == N.E and N.S in m for m in mixes)
    assert sum(c['all32'] for c in N.NECK.values()) >= 4


# ---- conditioning ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', N.neck_names())
def test_neck_oracle_is_well_conditioned(name):
    """FPN (four outputs), the chain and MultiStageMerging alone (both align_corners): fp32 vs fp64 max-rel < REL / 20.
    tiles_gt_cus on image 0 only (the oracle treats the images of a batch independently)."""
    c = N.NECK[name]
    images = (0, 1) if name == 'tiles_gt_cus' else None
    a, b = N.neck_oracle(c, torch.float32, images), N.neck_oracle(c, torch.float64, images)
    errs = [max_rel(x.double(), y) for x, y in zip(a['fpn'], b['fpn'])] + [max_rel(a['chain'].double(), b['chain'])]
    if c['msm']:
        errs += [max_rel(a['msm'][ac].double(), b['msm'][ac]) for ac in (False, True)]
    print(f'{name}: fp32 vs fp64 oracle max-rel {" ".join(f"{e:.2e}" for e in errs)} (cap {N.COND:.0e})')
    assert all(torch.isfinite(t).all() for t in b['fpn']) and max(errs) < N.COND


@pytest.mark.parametrize('name', list(N.FCN))
def test_fcn_oracle_is_well_conditioned(name):
    c = N.FCN[name]
    a, b = N.fcn_oracle(c, torch.float32), N.fcn_oracle(c, torch.float64)
    err = max_rel(a.double(), b)
    print(f'{name}: fp32 vs fp64 oracle max-rel {err:.2e} (cap {N.COND:.0e})')
    assert torch.isfinite(b).all() and float(b.abs().max()) > 0 and err < N.COND
    if c['dilation'] == 16 and (c['h'], c['w']) == (5, 7):
        # what the borders must do, stated independently: with the dilation beyond the map only the centre tap is inside
        z = N.fcn_oracle(c, torch.float64, centre=True)
        assert max_rel(b, z) < 1e-12


@pytest.mark.parametrize('name', list(N.LOOP))
def test_loop_oracle_is_well_conditioned_and_free_of_near_ties(name):
    """fp32 vs fp64 sampler around the FCN head: max-rel < REL / 20 and equal argmax; share of pixels whose top-2 margin of the
    OUTPUT is <= 1e-5 below 1e-3 (maps of < 1000 pixels: none)"""
    c = N.LOOP[name]
    a, b = N.loop_oracle(c, torch.float32), N.loop_oracle(c, torch.float64)
    assert a.shape == (c['B'], c['classes'], c['h'], c['w'])
    err = max_rel(a.double(), b)
    agree = float((a.argmax(1) == b.argmax(1)).float().mean())
    ties = N.top2_margin(a) <= N.MARGIN
    print(f'{name}: fp32 vs fp64 oracle max-rel {err:.2e} (cap {N.COND:.0e}), argmax equal {agree:.4f}, near-ties {int(ties.sum())} of {ties.numel()}')
    assert err < N.COND and agree == 1.0
    assert float(ties.float().mean()) < N.TIE_SHARE and (ties.numel() >= 1000 or not ties.any())


# ---- near-tie share of the epilogue cases ---------------------------------------------------------------------------------------
def _assert_ties(name, margin):
    ties = margin <= N.MARGIN
    print(f'{name}: {int(ties.sum())} of {ties.numel()} pixels within {N.MARGIN:g} of a tie')
    assert float(ties.float().mean()) < N.TIE_SHARE and (ties.numel() >= 1000 or not ties.any()), name


@pytest.mark.parametrize('name', N.epi_names('post'))
def test_post_cases_have_no_near_ties(name):
    c = N.EPI[name]
    sc = N.post_scores(c)
    p = N.post_probs(c, sc)
    fl = c['flip']
    assert torch.equal(p.argmax(1), O.seg_postprocess(sc, c['img'], c['crop'], c['out'], c['align'], fl))    # pinned to the oracle
    if c['K'] > 1:
        _assert_ties(name, N.top2_margin(p))


def test_aug_and_slide_cases_have_no_near_ties():
    c = N.EPI['aug_16']
    scores, metas = N.aug_inputs(c)
    assert len({(m['img_size'], m['flip']) for m in metas}) >= 8           # mixed sizes and flips
    _, p = O.seg_aug_test(scores, metas, c['out'], c['align'])
    _assert_ties('aug_16', N.top2_margin(p))
    c = N.EPI['slide_64']
    _, p = N.slide_oracle(c)
    assert p.shape == (c['B'], c['K']) + c['out']
    _assert_ties('slide_64', N.top2_margin(p))


# ---- workspace sums -------------------------------------------------------------------------------------------------------------
# The four sums below restate the layout functions of csrc/ddp_api.hip buffer by buffer.  They are a change detector (a buffer
# added, dropped or resized without the table of sizes here being revisited fails on the CPU), not an independent derivation of
# what the kernels need: that check is the guarded, NaN-filled, exactly sized workspace of tests/test_next_rows_gpu.py.
def _fpn_bytes(c, B):
    """fpn_layout: weight region (packed + split planes of the widest operand, per level the lateral and the 3x3 stage images),
    then per level input, conv output, lateral (whole 256-row tiles), statistics, partial sums in 32-token chunks"""
    max_w = max([2304] + c['channels'])
    n = _r256(256 * max_w * 4) + _r256(3 * 256 * max_w * 2)
    for ch in c['channels']:
        n += _r256(ch // 32 * N.STAGE_BYTES) + _r256(72 * N.STAGE_BYTES)
    for ch, (h, w) in zip(c['channels'], c['levels']):
        mp = _rows(B * h * w)
        n += _r256(mp * ch * 4) + 2 * _r256(mp * 256 * 4) + _r256(B * 64 * 4) + _r256(B * ((h * w + 31) // 32) * 64 * 8)
    return n


def _msm_bytes(c, B):
    """msm_layout: split planes of one 256 x 256 block, four times 8 stage images; per level input and conv output; the merged
    map's partial sums (32-token chunks of level 0) and statistics"""
    n = _r256(3 * 256 * 256 * 2) + 4 * _r256(8 * N.STAGE_BYTES)
    for h, w in c['levels']:
        n += 2 * _r256(_rows(B * h * w) * 256 * 4)
    h, w = c['levels'][0]
    return n + _r256(B * ((h * w + 31) // 32) * 64 * 8) + _r256(B * 64 * 4)


def _fcn_bytes(maps, h, w, K):
    """fcn_layout: row-major input, two fragment-major activations, the SB staging, packed and split 3x3 weights, 72 stage
    images, FiLM / affine / class-bias vectors, logits padded to 32 classes"""
    mp, ldl = _rows(maps * h * w), (K + 31) // 32 * 32
    return (3 * _r256(mp * 256 * 4) + _r256(mp * 256 * 6) + _r256(256 * 2304 * 4) + _r256(3 * 256 * 2304 * 2) + _r256(72 * N.STAGE_BYTES) +
            2 * _r256(512 * 4) + _r256(256 * 4) + _r256(mp * ldl * 4))


def _loop_bytes(c, B):
    """fcn_loop_layout: the head's workspace for B r maps, then the loop's buffers - B rows (xtok, xproj) and B r rows (mask,
    prob, step noise), one staging buffer for the larger padded operand, per (step, conv) 72 stage images and a shift vector"""
    r, K, Kc, Cx, nc = c['r'], c['K'], c['classes'], c['Cx'], c['num_convs']
    n_tok = c['h'] * c['w']
    mb, m = B * n_tok, B * r * n_tok
    ldl = (Kc + 31) // 32 * 32
    n = _fcn_bytes(B * r, c['h'], c['w'], Kc)
    n += _r256(_lib.MAX_STEPS * 4) + _r256(K * 17 * 4) + 2 * _r256(K * 1024 * 4) + _r256((Kc + 1) * 256 * 4)
    n += _r256(256 * Cx * 4) + _r256(256 * 256 * 4) + _r256(3 * 256 * Cx * 2) + _r256(3 * 256 * 256 * 2)
    n += _r256(mb * Cx * 4) + _r256(mb * 256 * 4) + _r256(m * 256 * 4) + _r256(m * ldl * 4)
    n += _r256(m * 256 * 4) if c['sampler'] == 'ddpm' else 0
    n += _r256(max(_rows(mb) * Cx, _rows(m) * 256) * 6)
    n += _r256(K * nc * 72 * N.STAGE_BYTES) + _r256(K * max(nc, 1) * 256 * 4) + _r256(8 * N.STAGE_BYTES) + _r256(256 * 4)
    return n


@pytest.mark.parametrize('name', N.neck_names())
def test_neck_workspace_is_the_sum_of_its_buffers(name):
    lib = _lib.load()
    c = N.NECK[name]
    for B in sorted({c['B'], 1}):
        fpn, msm, chain = N.neck_queries(lib, c, B)
        assert fpn == _fpn_bytes(c, B), (fpn, _fpn_bytes(c, B))
        assert msm == _msm_bytes(c, B), (msm, _msm_bytes(c, B))
        assert chain == fpn + msm


@pytest.mark.parametrize('name', list(N.FCN))
def test_fcn_workspace_is_the_sum_of_its_buffers(name):
    lib = _lib.load()
    c = N.FCN[name]
    for maps in sorted({c['maps'], 1}):
        assert N.fcn_query(lib, c, maps) == _fcn_bytes(maps, c['h'], c['w'], c['classes'])


@pytest.mark.parametrize('name', list(N.LOOP))
def test_loop_workspace_is_the_sum_of_its_buffers(name):
    lib = _lib.load()
    c = N.LOOP[name]
    for gemm in ('bf16x3', 'f32'):          # (cfg.gemm_mode is validated and otherwise unused by this loop: the same layout)
        for B in sorted({c['B'], 1}):
            assert N.loop_query(lib, c, gemm, B) == _loop_bytes(c, B), (gemm, B)


def test_limits_are_accepted_and_one_past_is_refused():
    """the C entries' own limits, from the accepting side (the GPU test runs them) and one past (DDP_E_BADCFG with a message)"""
    lib = _lib.load()
    n = C.c_size_t(0)
    for maps, h, w, k, ok in ((1, 1, 1, 1, True), (1, 1, 1, 256, True), (1, 1, 1, 257, False), (1, 1, 1, 0, False), (0, 1, 1, 19, False)):
        rc = lib.ddp_fcn_head_workspace(maps, h, w, k, C.byref(n))
        assert (rc == 0) == ok and (ok or (rc == -1 and b'fcn_head' in lib.ddp_last_error()))
    c = N.LOOP['max_steps']
    for nc, dil, ok in ((0, 1, True), (8, 1, True), (9, 1, False), (1, 0, False), (1, 64, True)):
        cfg = N.loop_cfg(c)
        rc = lib.ddp_sample_fcn_workspace(C.byref(cfg), nc, dil, C.byref(n))
        assert (rc == 0) == ok and (ok or rc == -1), (nc, dil, rc)
    cfg = N.loop_cfg(dict(c, K=_lib.MAX_STEPS + 1))
    assert lib.ddp_sample_fcn_workspace(C.byref(cfg), 1, 1, C.byref(n)) == -1 and b'timesteps' in lib.ddp_last_error()
    for ch, ok in ((64, True), (4096, True), (32, False), (4128, False), (80, False)):
        lv = N.fpn_level_structs(dict(N.NECK['chan_min'], channels=[ch] * 4), None)
        rc = lib.ddp_neck_fpn_workspace(lv, 1, C.byref(n))
        assert (rc == 0) == ok and (ok or (rc == -1 and b'channels' in lib.ddp_last_error())), ch


def test_a_coarser_level_larger_than_level_0_is_accepted():
    """levels 4x4, 8x8, 2x2, 1x1: the ABI does not forbid it and the layouts size every level from its own shape - the queries
    accept it (the GPU test asserts that the result is the oracle's: nearest / bilinear resizing in either direction)"""
    lib = _lib.load()
    c = N.NECK['coarse_larger']
    fpn, msm, chain = N.neck_queries(lib, c)
    assert fpn == _fpn_bytes(c, c['B']) and msm == _msm_bytes(c, c['B']) and chain == fpn + msm
