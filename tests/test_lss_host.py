"""CPU side of the device-side LSS lift and pool (tests/test_lss_gpu.py runs the cases on an MI355X): the fixtures recorded from the
reference's own ``LSSTransform`` equal the restatements of tests/lss_cases.py (ranks exactly); every case holds the witnesses its name
promises, counted in float64 - the synthetic rank tables of ``lss_cases.SYNTH`` included -; a restatement with ``floor`` instead of
truncation changes every kept mask; five wrong kernels (a pixel index modulo 64, channel groups read as zero, segment starts without
the tile starts, the last K % 4 counts dropped, list tails dropped), restated in float64, leave the bound; the near-boundary share
stays below 1 %; the library is a library of its own (exports, hash, stamp, ABI); every refusal happens before any launch; the
workspace formula; no kernel touches scratch; the device-free plugin surface.  No GPU compute is invoked."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import lss_cases as LC
from ddp_amd import _cm_lib, build, registry
from ddp_amd import _lss_lib as M
from ddp_amd import lss as L
from ddp_amd.bev.lss import LSSTransform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'lss')
WITNESSED = [n for n in LC.NAMES if n != 'empty']
SCAN_TILE, PRE_PIX = 1024, 64          # ddp_lss.hip: counts a block of the tiled scan owns; pixels a pre-pass block owns


# ---- fixture = restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', LC.NAMES)
def test_fixture_equals_the_restatement(name):
    c = LC.case(name)
    fix, ds2 = LC.load_fixture(name, GOLDEN)
    for k in ('img', 'camera2lidar', 'camera_intrinsics', 'img_aug_matrix', 'lidar_aug_matrix'):
        assert np.array_equal(fix[k], c[k].numpy()), k
    src = fix if 'geom' in fix.files else LC.load_fixture(LC.CASES[name]['same_points_as'], GOLDEN)[0]
    geom = torch.from_numpy(src['geom'])
    mine = LC.geometry_f32(c).reshape(-1, 3)
    assert geom.dtype == torch.float32 and geom.shape == (c['P'], 3)
    assert torch.allclose(mine, geom, rtol=1e-6, atol=1e-6)
    # ranks exactly: the reference's indices and kept mask against truncation of the fp32 cell coordinate, from the reference's own
    # geometry and from the restated chain
    for g in (geom, mine):
        r, kept = LC.ranks_of(c, LC.cells_f32(c, g))
        assert np.array_equal(r, fix['ranks']) and np.array_equal(kept, fix['kept']), name
    assert np.array_equal(fix['kept'], fix['ranks'] >= 0) and fix['ranks'].dtype == np.int32 and fix['ranks'].max() < c['K']
    # the geometry members and the state-dict entries the restatement rests on
    sd = LC.state_dict_of(fix)
    assert [int(v) for v in sd['nx']] == c['nx'] and sd['frustum'].shape == (c['D'], c['fH'], c['fW'], 3)
    assert torch.equal(sd['frustum'], LC.frustum_f32(c))
    dx, bx = LC.grid_f32(c)
    assert torch.equal(sd['dx'], dx) and torch.equal(sd['bx'], bx)
    # the pooled output (the generator's index_add_ stub, fp32) against the float64 sum over the same ranks, inside the bound
    x = LC.depthnet_out(c, sd['depthnet.weight'], sd['depthnet.bias'])
    logit = x[:, :c['D']]
    assert float((logit.max(1, keepdim=True).values - logit).max()) <= 16.0            # the bound's condition on the cases
    want, absum, Ls = LC.pool_f64(c, x.numpy(), fix['ranks'])
    assert fix['out'].shape == want.shape == (c['B'], c['nx'][2] * c['C'], c['nx'][0], c['nx'][1])
    assert (np.abs(fix['out'] - want) <= LC.pool_bound(c, absum, Ls)).all()
    assert (fix['out'][absum == 0] == 0).all()
    if ds2 is not None:
        assert c['nx'][2] == 1
        assert ds2['out'].shape == (c['B'], c['C'], (c['nx'][0] + 1) // 2, (c['nx'][1] + 1) // 2)
        assert np.array_equal(ds2['sd/depthnet.weight'], fix['sd/depthnet.weight'])
    else:
        assert c['nx'][2] > 1 and not os.path.exists(os.path.join(GOLDEN, f'lss_{name}_ds2.npz'))


# ---- witnesses -----------------------------------------------------------------------------------------------------------------------
def _witness(name):
    c = LC.case(name)
    q = LC.cells_f64(c)
    r, kept = LC.ranks_of(c, q)
    return c, q, r, kept


@pytest.mark.parametrize('name', WITNESSED)
def test_every_case_has_its_witnesses(name):
    c, q, r, kept = _witness(name)
    s = c['spec']
    nx = np.array(c['nx'])
    assert (kept & ((q > -1) & (q < 0)).any(1)).any()                      # a kept point with a coordinate in (-1, 0)
    beyond = {ax + '-': (q[:, a] <= -1) for a, ax in enumerate('xyz')}
    beyond.update({ax + '+': (q[:, a] >= nx[a]) for a, ax in enumerate('xyz')})
    # `tiny` has two points: one is the kept witness, the other is dropped beyond one face; every other case has all six
    assert s['faces'] == (['y+'] if name == 'tiny' else LC.ALL_FACES)
    for face in s['faces']:
        assert (beyond[face] & ~kept).any(), face
    lists = np.bincount(r[kept], minlength=c['K'])
    assert (lists == 0).any() and lists.max() >= s['longest'] >= 1
    assert lists.sum() == kept.sum() > 0


def test_each_name_keeps_its_promise():
    c, q, r, kept = _witness('tiny')
    assert (c['B'], c['N'], c['D'], c['fH'], c['fW'], c['C'], c['nx']) == (1, 1, 2, 1, 1, 1, [2, 2, 1]) and c['P'] == 2
    c, q, r, kept = _witness('odd')
    assert (c['B'], c['N'], c['D'], c['fH'], c['fW'], c['C'], c['nx']) == (2, 3, 13, 5, 7, 8, [16, 16, 2])
    z = (r[kept] // (16 * 16)) % 2
    assert (z == 0).any() and (z == 1).any()                               # both slabs hold points: the z * C + c order shows
    assert all(((r[kept] // (2 * 16 * 16)) == b).any() for b in (0, 1))
    assert LC.case('c3')['C'] == 3
    c, q, r, kept = _witness('cfg')
    assert (c['B'], c['N'], c['D'], c['fH'], c['fW'], c['C'], c['nx']) == (1, 6, 118, 4, 11, 80, [32, 32, 1])
    assert c['spec']['xbound'][2] == c['spec']['ybound'][2] == 3.2
    lng = LC.case('long')
    assert lng['nx'] == [2, 2, 1] and torch.equal(lng['img'], c['img']) and torch.equal(lng['camera2lidar'], c['camera2lidar'])
    lists = np.bincount(_witness('long')[2][_witness('long')[3]], minlength=4)
    assert lists.max() >= 1000 > 64                                        # longer than the 64 entries a wave takes at a time
    c = LC.case('runs')
    assert c['nx'][1] % LC.LSS_RUN != 0 and c['nx'][1] > LC.LSS_RUN
    c, q, r, kept = _witness('empty')
    assert not kept.any() and (r == -1).all()
    # past the first tile of every tiling of ddp_lss.hip (1024 cells per scan tile, 4 counts per thread, 64 pixels per pre-pass
    # block, 64 channels per pool group, 32 iy cells per pool block)
    c, q, r, kept = _witness('tiles')
    assert (c['B'], c['N'], c['D'], c['fH'], c['fW'], c['C'], c['nx']) == (2, 3, 10, 9, 15, 5, [45, 47, 1]) and c['P'] == 8100
    assert c['K'] == 4230 > 4 * SCAN_TILE and c['K'] % 4 == 2 and (c['K'] // 2) % SCAN_TILE != 0     # the second sample starts inside a tile
    assert c['fH'] * c['fW'] == 135 == 2 * PRE_PIX + 7
    assert sorted(set(r[kept] // SCAN_TILE)) == [0, 1, 2, 3, 4]
    assert sorted(set((np.flatnonzero(kept) % 135) // PRE_PIX)) == [0, 1, 2]
    assert sorted(set((r[kept] % 47) // LC.LSS_RUN)) == [0, 1] and sorted(set(r[kept] // 2115)) == [0, 1]
    lists = np.bincount(r[kept], minlength=c['K'])
    assert lists.max() > 64 and sorted(set(lists[lists > 0] % 4)) == [0, 1, 2, 3]
    for name, groups in (('c129', 3), ('c256', 4)):
        c, q, r, kept = _witness(name)
        HW, cells = c['fH'] * c['fW'], c['nx'][0] * c['nx'][1]
        assert (c['C'] + 63) // 64 == groups and HW > PRE_PIX and HW % PRE_PIX != 0 and c['nx'][2] == 2
        assert sorted(set(r[kept] // cells)) == [0, 1]                     # both slabs hold points
        assert (np.flatnonzero(kept) % HW >= PRE_PIX).any()
    assert LC.case('c129')['C'] == 2 * 64 + 1 and LC.case('c129')['fH'] * LC.case('c129')['fW'] == PRE_PIX + 1
    assert LC.case('c256')['C'] == M.MAX_CHANNELS and LC.case('c256')['K'] % 4 == 2
    # the synthetic rank tables: the exact list lengths, and the scan past one block's 1024 tile sums
    assert [LC.SYNTH[n]['C'] for n in LC.SYNTH_NAMES if n.startswith('lens_')] == [64, 65, 128, 192, 193]
    for name in LC.SYNTH_NAMES:
        c = LC.synth(name)
        kept = c['ranks'] >= 0
        lists = np.bincount(c['ranks'][kept], minlength=c['K'])
        assert c['K'] % 4 == 3 and c['x'].shape == (1, c['D'] + c['C'], c['fH'], c['fW']) and c['x'].dtype == torch.float32
        assert float(c['x'].max() - c['x'].min()) <= 4.0
        if name == 'scan':
            assert (c['D'], c['fH'] * c['fW'], c['P'], c['C'], c['nx']) == (4, 16 * PRE_PIX, 4096, 1, [1, 1048579, 1])
            tiles = (c['K'] + SCAN_TILE - 1) // SCAN_TILE
            assert tiles == 1025 and (tiles + 1023) // 1024 == 2 and c['K'] - 1024 * SCAN_TILE == 3
            assert all(lists[cell] >= 1 for cell in (0, 1023, 1024, 1048575, 1048576, 1048577, 1048578))
            assert (lists > 0).sum() == 7 + 600 and lists.sum() == 15 + 600
        else:
            assert (c['D'], c['fH'] * c['fW'], c['P'], c['nx'], c['K']) == (16, 72, 1152, [3, 37, 1], 111)
            assert {int(k): int(lists[k]) for k in np.flatnonzero(lists)} == LC.LENS == {
                0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 31: 7, 32: 8, 36: 63, 37: 64, 73: 65, 74: 127, 107: 128, 108: 129, 109: 1, 110: 3}
            assert lists.sum() == 610 and np.array_equal(c['ranks'], LC.synth('lens_c64')['ranks'])          # one table
            assert 36 % 37 == 36 and 37 % 37 == 0 and 37 - LC.LSS_RUN == 5                                     # row edge; a run of 5 cells
        for cell in np.flatnonzero(lists >= 3):                            # dealt through a permutation: no list is a run of ids
            assert (np.diff(np.flatnonzero(c['ranks'] == cell)) > 1).any(), cell


def test_no_lss_fixture_outgrows_the_largest_of_the_first_set():
    sizes = {f: os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.endswith('.npz')}
    assert len(sizes) == 17 and max(sizes.values()) == sizes['lss_cfg.npz'] == 451541, sizes


# ---- what a wrong kernel would show: each variant, restated in float64, leaves the bound on the case that is there for it ---------------
def _pool_inputs(name):
    if name in LC.SYNTH:
        c = LC.synth(name)
        return c, c['x'].numpy(), c['ranks']
    c = LC.case(name)
    fix = LC.load_fixture(name, GOLDEN)[0]
    return c, LC.depthnet_out(c, fix['sd/depthnet.weight'], fix['sd/depthnet.bias']).numpy(), fix['ranks']


def _pixel_modulo_64(c, x, ranks):
    """(a) the pre-pass forgets its tile: pixel px reads pixel px % 64"""
    px = np.arange(c['fH'] * c['fW']) % PRE_PIX
    return x.reshape(x.shape[0], x.shape[1], -1)[:, :, px].reshape(x.shape), ranks


def _channels_from(first):
    def mutate(c, x, ranks):
        """(b) the pool's channel groups past ``first`` read as zero"""
        x = x.copy()
        x[:, c['D'] + first:] = 0.0
        return x, ranks
    return mutate


def _last_counts_dropped(c, x, ranks):
    """(d) the scan drops the last K % 4 counts: those cells' lists are empty"""
    return x, np.where(ranks >= c['K'] - c['K'] % 4, -1, ranks).astype(np.int32)


def _list_tails_dropped(c, x, ranks):
    """(e) the pool walks four entries at a time and forgets the rest: the last L % 4 entries of every list"""
    ranks = ranks.copy()
    for cell in np.unique(ranks[ranks >= 0]):
        ids = np.flatnonzero(ranks == cell)
        ranks[ids[ids.size - ids.size % 4:]] = -1
    return x, ranks


WRONG = ([('pixel % 64', _pixel_modulo_64, n) for n in ('tiles', 'c129')]
         + [(f'channels from {first} zero', _channels_from(first), n) for n, first in (('c129', 128), ('c256', 128), ('c256', 192),
                                                                                      ('lens_c193', 128), ('lens_c193', 192))]
         + [('last K % 4 counts dropped', _last_counts_dropped, n) for n in LC.SYNTH_NAMES if n.startswith('lens_')]
         + [('list tails dropped', _list_tails_dropped, n) for n in LC.SYNTH_NAMES if n.startswith('lens_')])


@pytest.mark.parametrize('what,mutate,name', WRONG, ids=[f'{w}-{n}' for w, _, n in WRONG])
def test_a_wrong_pool_leaves_the_bound(what, mutate, name):
    c, x, ranks = _pool_inputs(name)
    want, absum, lists = LC.pool_f64(c, x, ranks)
    bound = LC.pool_bound(c, absum, lists)
    got = LC.pool_f64(c, *mutate(c, x, ranks))[0]
    assert (np.abs(got - want) > bound).any(), (what, name)
    assert (np.abs(LC.pool_f64(c, x.copy(), ranks.copy())[0] - want) <= bound).all()          # and the restatement itself stays inside


@pytest.mark.parametrize('name', ['tiles', 'scan'])
def test_segment_starts_without_the_tile_starts_are_wrong(name):
    """(c) the tiled scan forgets ``sums[tile]``: the starts of every tile begin at zero again.  Offsets compared, not the pool."""
    c, x, ranks = _pool_inputs(name)
    lists = np.bincount(ranks[ranks >= 0], minlength=c['K']).astype(np.int64)
    starts = np.cumsum(lists) - lists
    tile = np.arange(c['K']) // SCAN_TILE
    local = starts - starts[tile * SCAN_TILE]
    assert tile.max() >= 4 and np.array_equal(local[:SCAN_TILE], starts[:SCAN_TILE])
    wrong = np.flatnonzero((local != starts) & (lists > 0))               # a non-empty cell whose list would be read from elsewhere
    assert wrong.size and set(tile[wrong]) == set(tile[(lists > 0) & (tile > 0)])
    # and the lengths alone do not show it: np.diff of the wrong starts differs from the counts only at tile starts
    diff = np.diff(np.append(local, local[-1] + lists[-1]))
    assert set(np.flatnonzero(diff != lists)) <= set(np.arange(SCAN_TILE, c['K'], SCAN_TILE) - 1)


@pytest.mark.parametrize('name', WITNESSED)
def test_floor_instead_of_truncation_changes_the_kept_mask(name):
    """the quirk is pinned: `.long()` truncates toward zero, so a coordinate in (-1, 0) is cell 0 and kept; floor drops it"""
    c, q, r, kept = _witness(name)
    rf, keptf = LC.ranks_of(c, q, mode='floor')
    assert (kept != keptf).any() and not (keptf & ~kept).any()
    fix = LC.load_fixture(name, GOLDEN)[0]
    rf32, keptf32 = LC.ranks_of(c, LC.cells_f32(c), mode='floor')
    assert not np.array_equal(keptf32, fix['kept']) and not np.array_equal(rf32, fix['ranks'])


@pytest.mark.parametrize('name', LC.NAMES)
def test_near_boundary_share(name):
    c, q, r, kept = _witness(name)
    near = LC.near_boundary(q)
    assert near.mean() <= LC.EXCUSED_SHARE and LC.DELTA == 1e-3
    # a point away from every boundary has one admissible rank, its own
    ok = LC.admissible(c, q, r)
    assert ok.all()
    wrong = np.where(r >= 0, -1, 0).astype(np.int32)
    assert not LC.admissible(c, q, wrong)[~near].any()
    # the fp32 restatement sits far inside DELTA of the float64 one
    assert np.abs(LC.cells_f32(c) - q).max() < LC.DELTA / 10
    assert LC.admissible(c, q, LC.ranks_of(c, LC.cells_f32(c))[0]).all()


# ---- the library's own (what every side library shares: tests/test_build_host.py) ------------------------------------------------------
def test_binding_matches_the_header():
    build.SIDE['lss'].start(verbose=False)()
    header = open(os.path.join(ROOT, 'include', 'ddp_lss_mi355x.h')).read()
    assert '#define DDP_LSS_MAX_CHANNELS 256' in header and '#define DDP_LSS_MAX_DEPTH_BINS 512' in header
    assert (M.MAX_CHANNELS, M.MAX_DEPTH_BINS) == (256, 512)
    assert (M.E_BADCFG, M.E_ALIGN, M.E_LAUNCH, M.E_NULL) == (_cm_lib.E_BADCFG, _cm_lib.E_ALIGN, _cm_lib.E_LAUNCH, _cm_lib.E_NULL)
    assert C.sizeof(M.Cfg) == 8 * 4 + 12 * 8 + 3 * 4 + 4                  # 8 ints, 12 doubles, nx[3], tail padding


def test_stale_or_missing_library_raises(tmp_path, monkeypatch):
    with pytest.raises(M.DdpLssError, match='not found'):
        M.load(str(tmp_path / 'libddp_lss.so'))
    monkeypatch.setattr(M._binding, 'libs', {})
    with monkeypatch.context() as m:
        m.setattr(build.SIDE['lss'], 'built_hash', lambda: 'feedfeedfeedfeed')
        with pytest.raises(M.DdpLssError, match='is stale'):
            M.load()
    monkeypatch.setattr(M._binding, 'abi_version', M.ABI_VERSION + 1)
    with pytest.raises(M.DdpLssError, match='ABI mismatch: library 1 vs binding 2') as e:
        M.load()
    assert e.value.code is None and isinstance(e.value, RuntimeError) and not M._binding.libs


FAKE = 0x10000    # a non-NULL, 256-byte aligned "device pointer": every call below is refused before anything is enqueued


def _cfg(**over):
    c = LC.case('odd')
    pool = L.LssPool(c['spec']['image'], c['spec']['feature'], c['spec']['xbound'], c['spec']['ybound'], c['spec']['zbound'],
                     c['spec']['dbound'], c['C'])
    cfg = pool.cfg(c['B'], c['N'])
    for k, v in over.items():
        if isinstance(v, (list, tuple)):
            getattr(cfg, k)[:] = v
        else:
            setattr(cfg, k, v)
    return cfg


def _calls(cfg, cam=FAKE, extra=FAKE, ws=FAKE, ranks=FAKE, x=FAKE, out=FAKE):
    lib = M.load()
    n, p = C.c_size_t(0), C.c_void_p(0)
    return dict(workspace=lambda: lib.ddp_lss_workspace(C.byref(cfg), C.byref(n)),
                plan=lambda: lib.ddp_lss_plan(C.byref(cfg), cam, extra, ws, None),
                plan_from_ranks=lambda: lib.ddp_lss_plan_from_ranks(C.byref(cfg), ranks, ws, None),
                ranks=lambda: lib.ddp_lss_ranks(C.byref(cfg), ws, C.byref(p)),
                pool=lambda: lib.ddp_lss_pool(C.byref(cfg), x, ws, out, None))


def _refused(rc, code, words):
    msg = M.load().ddp_lss_last_error().decode()
    assert rc == code and words in msg, (rc, msg)


def test_refusals_happen_before_any_launch():
    """no GPU is present where this runs: a call that got as far as a launch would fail with DDP_LSS_E_LAUNCH, not with these"""
    bad = [(dict(channels=0), 'channels 0 out of range [1,256]'), (dict(channels=257), 'channels 257'),
           (dict(depth_bins=0), 'depth_bins 0 out of range [1,512]'), (dict(depth_bins=513), 'depth_bins 513'),
           (dict(batch=0), 'batch'), (dict(cams=-1), 'cams'), (dict(feat_h=0), 'feat_h'), (dict(feat_w=0), 'feat_w'),
           (dict(image_h=0), 'image_h'), (dict(image_w=-3), 'image_w'), (dict(nx=[0, 4, 1]), 'nx[0]'), (dict(nx=[4, 0, 1]), 'nx[1]'),
           (dict(nx=[4, 4, 0]), 'nx[2]'), (dict(xbound=[0.0, 1.0, 0.0]), 'xbound'), (dict(dbound=[1.0, 2.0, float('nan')]), 'dbound'),
           (dict(zbound=[0.0, float('inf'), 1.0]), 'zbound'), (dict(ybound=[0.0, 1.0, -1.0]), 'ybound'),
           (dict(batch=1 << 12, cams=1 << 6, depth_bins=512, feat_h=8, feat_w=2), 'B*N*D*fH*fW'),          # = 2^31
           (dict(batch=65535, cams=1, depth_bins=512, feat_h=64, feat_w=1), 'B*N*D*fH*fW'),                # just below 2^31 passes this check ...
           (dict(batch=1 << 11, nx=[1 << 10, 1 << 10, 1]), 'B*nz*nx0*nx1'), (dict(nx=[46341, 46341, 1]), 'B*nz*nx0*nx1')]
    for over, words in bad:
        cfg = _cfg(**over)
        if over.get('batch') == 65535:                                     # ... 65535 * 512 * 64 = 2^31 - 32768: accepted
            n = C.c_size_t(0)
            assert M.load().ddp_lss_workspace(C.byref(cfg), C.byref(n)) == 0 and n.value > 4 * (2 ** 31 - 32768) * 4
            continue
        for name, call in _calls(cfg).items():
            _refused(call(), M.E_BADCFG, words)
    cfg = _cfg()
    for kw, name, what in ((dict(cam=None), 'plan', 'd_cam'), (dict(extra=None), 'plan', 'd_extra'), (dict(ws=None), 'plan', 'd_workspace'),
                           (dict(ranks=None), 'plan_from_ranks', 'd_ranks'), (dict(ws=None), 'plan_from_ranks', 'd_workspace'),
                           (dict(ws=None), 'ranks', 'd_workspace'), (dict(x=None), 'pool', 'd_depthnet_out'), (dict(ws=None), 'pool', 'd_workspace'),
                           (dict(out=None), 'pool', 'd_out')):
        _refused(_calls(cfg, **kw)[name](), M.E_NULL, what + ' is NULL')
    for kw, name, what in ((dict(cam=FAKE + 2), 'plan', 'd_cam'), (dict(extra=FAKE + 1), 'plan', 'd_extra'), (dict(ws=FAKE + 128), 'plan', 'd_workspace'),
                           (dict(ranks=FAKE + 2), 'plan_from_ranks', 'd_ranks'), (dict(ws=FAKE + 16), 'ranks', 'd_workspace'),
                           (dict(x=FAKE + 3), 'pool', 'd_depthnet_out'), (dict(ws=FAKE + 64), 'pool', 'd_workspace'), (dict(out=FAKE + 2), 'pool', 'd_out')):
        _refused(_calls(cfg, **kw)[name](), M.E_ALIGN, what + ' must be')
    lib = M.load()
    _refused(lib.ddp_lss_workspace(None, C.byref(C.c_size_t(0))), M.E_NULL, 'cfg is NULL')
    _refused(lib.ddp_lss_workspace(C.byref(cfg), None), M.E_NULL, 'bytes is NULL')
    _refused(lib.ddp_lss_ranks(C.byref(cfg), FAKE, None), M.E_NULL, 'd_ranks is NULL')
    # the binding turns a refused configuration into ValueError, anything else into DdpLssError
    with pytest.raises(ValueError, match='channels 257'):
        L.LssPool((256, 704), (4, 11), (-8, 8, 1), (-8, 8, 1), (-1, 1, 2), (1, 5, 1), 257)
    with pytest.raises(M.DdpLssError, match='is NULL') as e:
        M.check(_calls(cfg, ws=None)['pool'](), lib)
    assert e.value.code == M.E_NULL


def test_workspace_formula_and_rank_table_place():
    lib = M.load()
    for name in LC.NAMES + LC.SYNTH_NAMES:                                 # the synthetic bounds make LssPool derive the stated nx and D
        c = LC.synth(name) if name in LC.SYNTH else LC.case(name)
        s = c['spec']
        pool = L.LssPool(s['image'], s['feature'], s['xbound'], s['ybound'], s['zbound'], s['dbound'], c['C'])
        assert (pool.D, pool.nx, pool.C) == (c['D'], c['nx'], c['C'])
        for B, N in ((c['B'], c['N']), (3, 5)):
            assert pool.workspace_bytes(B, N) == LC.workspace_bytes(c, B, N)
            p = C.c_void_p(0)
            assert lib.ddp_lss_ranks(C.byref(pool.cfg(B, N)), FAKE, C.byref(p)) == 0 and p.value == FAKE
    # the configuration's size: 6 x 118 x 32 x 88 points, 256 x 256 cells, 80 channels
    pool = L.LssPool((256, 704), (32, 88), (-51.2, 51.2, 0.4), (-51.2, 51.2, 0.4), (-10.0, 10.0, 20.0), (1.0, 60.0, 0.5), 80)
    assert (pool.D, pool.nx) == (118, [256, 256, 1])
    P, K, X = 6 * 118 * 32 * 88, 65536, 6 * 32 * 88
    assert pool.workspace_bytes(1, 6) == 4 * 4 * P + 4 * K + 256 + 4 * K + 256 + 4 * X * 80 == 37831168


# ---- kernel resources ----------------------------------------------------------------------------------------------------------------
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_no_kernel_touches_scratch(tmp_path):
    out = tmp_path / 'lss.s'
    src = os.path.join(build.SIDE['lss'].csrc, 'ddp_lss.hip')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-x', 'hip', src,
                    '--cuda-device-only', '-S', '-o', str(out)], check=True, capture_output=True, timeout=600)
    figures = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', out.read_text(), re.S):
        body = m.group(2)
        short = re.search(r'k_lss_[a-z_]+(ILi\d)?', m.group(1)).group(0)
        figures[short] = tuple(int(re.search(rf'\.amdhsa_{key} (\d+)', body).group(1))
                               for key in ('private_segment_fixed_size', 'next_free_vgpr', 'group_segment_fixed_size'))
    print('kernel: (scratch B, VGPRs, static LDS B)', figures)
    assert sorted(figures) == sorted(['k_lss_rank', 'k_lss_take_ranks', 'k_lss_scan', 'k_lss_tile_sums', 'k_lss_tile_scan', 'k_lss_fill', 'k_lss_sort', 'k_lss_pre',
                                      'k_lss_poolILi1', 'k_lss_poolILi2', 'k_lss_poolILi3', 'k_lss_poolILi4'])
    for name, (scratch, vgpr, lds) in figures.items():
        assert scratch == 0, f'{name}: {scratch} B of scratch'
        assert vgpr <= 64, f'{name}: {vgpr} registers (eight waves per SIMD need <= 64)'
        assert lds <= 20 * 1024
    # the pooling kernel's dynamic LDS: [C][run + 1] floats, at most 33 KiB
    assert 256 * (LC.LSS_RUN + 1) * 4 <= 64 * 1024


# ---- plugin surface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['odd', 'cfg', 'tiny'])
def test_plugin_surface_is_the_reference_class(name):
    c = LC.case(name)
    fix, ds2 = LC.load_fixture(name, GOLDEN)
    assert registry.VTRANSFORMS is registry.MODELS and registry.MODELS.get('LSSTransform') is LSSTransform
    for ds, f in ((1, fix), (2, ds2)):
        if f is None:
            continue
        m = registry.VTRANSFORMS.build(dict(type='LSSTransform', downsample=ds, **c['kwargs']))
        sd = LC.state_dict_of(f)
        assert list(m.state_dict()) == list(sd)                           # the reference's keys, in its order
        assert all(m.state_dict()[k].shape == v.shape and m.state_dict()[k].dtype == v.dtype for k, v in sd.items())
        m.load_state_dict(sd, strict=True)
        assert m.D == c['D'] and m.C == c['C'] and [int(v) for v in m.nx] == c['nx'] and m.nx.dtype == torch.int64
        assert torch.equal(m.frustum, LC.frustum_f32(c)) and not m.frustum.requires_grad
        assert isinstance(m.depthnet, torch.nn.Conv2d) and m.depthnet.out_channels == c['D'] + c['C'] and m.depthnet.kernel_size == (1, 1)
        assert isinstance(m.downsample, torch.nn.Identity if ds == 1 else torch.nn.Sequential)
        assert 'pooler' not in dict(m.named_modules())
    # nx and D by the reference's expressions, not by rounding: (hi - lo) / step truncated, len(arange)
    assert [int(v) for v in L.grid_of((-51.2, 51.2, 0.4), (-51.2, 51.2, 0.4), (-10.0, 10.0, 20.0))[2]] == [256, 256, 1]
    assert [int(v) for v in L.grid_of((0.0, 0.7, 0.1), (0.0, 0.3, 0.1), (0.0, 1.0, 0.3))[2]] == [int(0.7 / 0.1), int(0.3 / 0.1), 3] == [6, 2, 3]
    assert L.depth_bins_of((1.0, 60.0, 0.5)) == 118 and L.depth_bins_of((2.0, 6.0, 2.0)) == 2
    import inspect
    assert list(inspect.signature(LSSTransform.__init__).parameters)[1:] == ['in_channels', 'out_channels', 'image_size', 'feature_size',
                                                                              'xbound', 'ybound', 'zbound', 'dbound', 'downsample']
    assert list(inspect.signature(LSSTransform.forward).parameters)[1:12] == [
        'img', 'points', 'camera2ego', 'lidar2ego', 'lidar2camera', 'lidar2image', 'camera_intrinsics', 'camera2lidar', 'img_aug_matrix',
        'lidar_aug_matrix', 'metas']


def test_cpu_tensors_raise():
    c = LC.case('c3')
    s = c['spec']
    pool = L.LssPool(s['image'], s['feature'], s['xbound'], s['ybound'], s['zbound'], s['dbound'], c['C'])
    with pytest.raises(ValueError, match='no CPU path'):
        pool.plan(torch.zeros(1, 2, 24), torch.zeros(1, 12))
    with pytest.raises(ValueError, match='no CPU path'):
        pool.plan_from_ranks(torch.zeros(1, 2, c['D'], 3, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r'\(B, N, 24\)'):
        pool.plan(torch.zeros(2, 24), torch.zeros(1, 12))
    with pytest.raises(RuntimeError, match='no plan'):
        pool.pool(torch.zeros(2, c['D'] + 3, 3, 4))
    with pytest.raises(RuntimeError, match='no plan'):
        pool.ranks()
    m = LSSTransform(**c['kwargs'])
    with pytest.raises(ValueError, match='no CPU path'):
        m(*LC.forward_args(c))
    cam, extra = L.pack_cameras(c['camera2lidar'][..., :3, :3], c['camera2lidar'][..., :3, 3], c['camera_intrinsics'][..., :3, :3],
                                c['img_aug_matrix'][..., :3, :3], c['img_aug_matrix'][..., :3, 3], c['lidar_aug_matrix'][..., :3, :3],
                                c['lidar_aug_matrix'][..., :3, 3])
    assert cam.shape == (1, 2, 24) and extra.shape == (1, 12) and cam.dtype == torch.float32
    assert torch.equal(cam[0, 0, :9].view(3, 3), torch.inverse(c['img_aug_matrix'][0, 0, :3, :3]))
    assert torch.equal(cam[0, 1, 9:12], c['img_aug_matrix'][0, 1, :3, 3]) and torch.equal(cam[0, 1, 21:], c['camera2lidar'][0, 1, :3, 3])
