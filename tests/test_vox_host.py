"""CPU side of the device-side hard voxelisation (tests/test_zz_vox_gpu.py runs the cases on an MI355X): the fixtures recorded from the
reference's own ``hard_voxelize_cpu`` and ``BEVFusion.voxelize`` equal the restatements of tests/vox_cases.py bit for bit (the means:
inside the derived bound); every case holds the witness its name promises; the binding matches the header; every refusal happens
before any launch; the workspace formula, which knows no grid volume; the documented hash; no kernel touches scratch; the device-free
plugin surface and ``use_device_voxelization`` on stub models.  No GPU compute is invoked."""
import ctypes as C
import inspect
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import vox_cases as VC
from ddp_amd import _cm_lib, build, registry
from ddp_amd import _vox_lib as M
from ddp_amd import vox as L
from ddp_amd.bev.voxelize import Voxelization

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'vox')


# ---- fixture = restatement -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', VC.FIXTURES)
def test_fixture_equals_the_restatement_bit_for_bit(name):
    c, fix = VC.case(name), VC.load_fixture(name, GOLDEN)
    assert json.loads(str(fix['config'])) == json.loads(VC.config_of(c)) and c['grid'][0] == c['grid'][2]
    assert os.path.getsize(os.path.join(GOLDEN, f'vox_{name}.npz')) <= 128 * 1024
    for b, p in enumerate(c['points']):
        assert fix[f'points{b}'].tobytes() == p.tobytes() and p.shape == (c['counts'][b], c['stride'])
        voxels, coors, num = VC.hard_voxelize_ref(p, c)
        assert fix[f'voxels{b}'].dtype == np.float32 and fix[f'coors{b}'].dtype == np.int32 and fix[f'num{b}'].dtype == np.int32
        assert fix[f'voxels{b}'].shape == voxels.shape and fix[f'voxels{b}'].tobytes() == voxels.tobytes()     # +0.0 in the unused slots
        assert np.array_equal(fix[f'coors{b}'], coors) and np.array_equal(fix[f'num{b}'], num)
    feats, coords, sizes = VC.batch_ref(c, reduce=True)
    raw = VC.batch_ref(c, reduce=False)[0]
    assert fix['coords'].dtype == np.int32 and np.array_equal(fix['coords'], coords) and fix['coords'].shape == (len(sizes), 4)
    assert np.array_equal(fix['sizes'], sizes) and fix['feats_raw'].tobytes() == raw.tobytes()
    assert fix['feats'].shape == feats.shape == (len(sizes), c['F'])
    # the means: torch's sum over the slot axis is not pinned to left-to-right, so both are held to the bound around float64
    want, bound = VC.mean_f64(raw, sizes)
    worst = {}
    for what, got in (('fixture', fix['feats']), ('restatement', feats)):
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), what
        worst[what] = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f'{name}: largest |fp32 mean - f64| / bound: {worst}; fixture means equal the left-to-right sum bit for bit: '
          f'{fix["feats"].tobytes() == feats.tobytes()}')


def test_the_restatement_follows_the_grid_rule_of_the_module():
    for g in (VC.G16, VC.G_EDGES, VC.G32, VC.G_FLAT, VC.G_RECIPE):
        assert [int(v) for v in L.grid_of(g['voxel_size'], g['range'])] == g['grid'] == VC.grid_of(g['voxel_size'], g['range'])
    assert VC.G_FLAT['grid'] == [40, 40, 8] and VC.G_RECIPE['grid'] == [1024, 1024, 40]
    assert [n for n in VC.NAMES if VC.case(n)['grid'][0] != VC.case(n)['grid'][2]] == ['flat'] and 'flat' not in VC.FIXTURES


# ---- witnesses -----------------------------------------------------------------------------------------------------------------------
def _tables(c, b=0):
    cells = VC.cells_ref(c['points'][b], c)
    return (cells,) + VC.assign_ref(cells, c['T'], c['max_voxels'])


def test_each_name_keeps_its_promise():
    c = VC.case('one')
    assert c['counts'] == [1] and len(VC.hard_voxelize_ref(c['points'][0], c)[0]) == 1
    c = VC.case('empty')
    assert c['counts'] == [0] and VC.hard_voxelize_ref(c['points'][0], c)[0].shape == (0, 3, 5)
    c = VC.case('all_out')
    assert c['counts'] == [7] and (VC.cells_ref(c['points'][0], c) == -1).all()
    # edges: on every axis the bounds, their neighbours and a lattice plane; -0.0 is in cell 0; hi is out, its lower neighbour in
    c = VC.case('edges')
    assert c['counts'] == [200] and c['grid'] == [16, 24, 16] and sorted(set(c['voxel_size'])) == [0.075, 0.1]
    cells, p = VC.cells_ref(c['points'][0], c), c['points'][0]
    lo, hi = np.asarray(c['range'][:3], np.float32), np.asarray(c['range'][3:], np.float32)
    for j in range(3):
        col, rows = p[10 * j:10 * j + 10, j], cells[10 * j:10 * j + 10]
        # lo is in, its lower neighbour out, hi and its upper neighbour out; where the fp32 quotient puts the LOWER neighbour of hi and of
        # a lattice plane - it may round up onto the plane - is the reference's bits' to say (the fixture)
        assert col[0] == lo[j] and col[3] == hi[j] and rows[0] >= 0 and rows[1] == -1 and rows[2] == rows[0] and rows[3] == -1 and rows[5] == -1
        assert rows[6] >= 0 and rows[7] >= 0 and rows[8] == rows[6]
    assert sum(int(cells[10 * j + 6] != cells[10 * j + 7]) + int(cells[10 * j + 4] >= 0) for j in range(3)) >= 1
    assert np.signbit(p[9, 0]) and p[9, 0] == 0 and cells[9] >= 0 and cells[9] // (24 * 16) == 0
    onl = ((p[:, :3] - lo) / np.asarray(c['voxel_size'], np.float32))
    assert (onl == np.floor(onl)).all(1).sum() >= 50                       # points on lattice corners
    # nonfinite: the 15 rows are dropped, their neighbours stay
    c = VC.case('nonfinite')
    cells, p = VC.cells_ref(c['points'][0], c), c['points'][0]
    bad = ~np.isfinite(p[:, :3]).all(1) | (np.abs(p[:, :3]) > 1e29).any(1)
    assert c['counts'] == [64] and bad.sum() == 15 and (cells[bad] == -1).all() and (cells[~bad] >= 0).all()
    assert all(np.isnan(p[:, j]).sum() == 1 and np.isinf(p[:, j]).sum() == 2 and (np.abs(p[:, j]) == np.float32(1e30)).sum() == 2 for j in range(3))
    # dups: five cells of 60 points each, dealt: the first three of a voxel are not its first three neighbours in memory
    c = VC.case('dups')
    cells, pvox, table, vcells = _tables(c)
    assert c['counts'] == [300] and c['T'] == 3 and len(table) == 5 and (np.bincount(pvox) == 60).all()
    assert (np.diff(table, axis=1) > 0).all() and (np.diff(table, axis=1) > 1).any() and table[:, 0].tolist() == sorted(table[:, 0].tolist())
    c = VC.case('one_voxel')
    cells, pvox, table, vcells = _tables(c)
    assert c['counts'] == [20000] and c['T'] == 10 and len(set(cells.tolist())) == 1 and table.tolist() == [list(range(10))]
    # cap: more cells than voxels; a kept voxel gains a point after the cap was hit; dropped cells come back later and stay dropped
    c = VC.case('cap')
    cells, pvox, table, vcells = _tables(c)
    first_dropped = int(np.flatnonzero((pvox == -1) & (cells >= 0))[0])
    assert c['counts'] == [1000] and len(set(cells.tolist())) == 400 and c['max_voxels'] == 37 == len(table)
    assert (pvox[first_dropped:] >= 0).sum() >= 1 and ((table > first_dropped).sum() >= 1)
    assert len(vcells) == len(set(vcells.tolist())) and vcells.tolist() == list(dict.fromkeys(cells[cells >= 0].tolist()))[:37]
    for d in (-1, 0, 1):
        c = VC.case(f'cap_exact{d:+d}')
        cells, pvox, table, vcells = _tables(c)
        assert len(set(cells.tolist())) == 40 and c['max_voxels'] == 40 + d and len(table) == min(40, 40 + d)
        assert ((pvox == -1).sum() > 0) == (d == -1)
    for n in VC.TILES:
        c = VC.case(f'tiles{n}')
        cells, pvox, table, vcells = _tables(c)
        founders = table[:, 0]
        assert c['counts'] == [n] and founders[-1] == n - 1 and len(table) < c['max_voxels']            # the last point founds the last voxel
        assert len(set((founders // M.SCAN_TILE).tolist())) == (n + M.SCAN_TILE - 1) // M.SCAN_TILE and (cells == -1).any()
    assert {n % M.SCAN_TILE for n in VC.TILES} == {0, 1, M.SCAN_TILE - 1} and M.SCAN_TILE + 1 in VC.TILES
    for F, pad in VC.FEATS:
        c = VC.case(f'feat{F}+{pad}')
        assert (c['F'], c['stride']) == (F, F + pad) and c['points'][0].shape == (150, F + pad)
    assert {F for F, _ in VC.FEATS} == {3, 4, 5, M.MAX_FEATS}
    c = VC.case('batch')
    per = [VC.hard_voxelize_ref(p, c) for p in c['points']]
    feats, coords, sizes = VC.batch_ref(c)
    assert c['B'] == 3 and c['counts'][1] == 0 and c['counts'][0] != c['counts'][2] and len(per[1][0]) == 0
    assert 0 < len(per[0][0]) < c['max_voxels'] == len(per[2][0]) and coords[-1, 0] + 1 == 3 and sorted(set(coords[:, 0].tolist())) == [0, 2]
    assert (sizes == c['T']).any() and (sizes == 1).any()


# ---- the binding and the header ------------------------------------------------------------------------------------------------------
def test_binding_matches_the_header():
    build.LATER['vox'].start(verbose=False)()
    header = open(os.path.join(ROOT, 'include', 'ddp_vox_mi355x.h')).read()
    for k, v in (('WS_ALIGN', M.WS_ALIGN), ('MAX_FEATS', M.MAX_FEATS), ('MAX_POINTS', M.MAX_POINTS), ('SCAN_TILE', M.SCAN_TILE)):
        assert re.search(rf'#define DDP_VOX_{k} {v}\b', header), k
    assert f'#define DDP_VOX_HASH_MULT {M.HASH_MULT}u' in header
    assert (M.E_BADCFG, M.E_ALIGN, M.E_LAUNCH, M.E_NULL) == (_cm_lib.E_BADCFG, _cm_lib.E_ALIGN, _cm_lib.E_LAUNCH, _cm_lib.E_NULL)
    assert 'DDP_VOX_E_BADCFG = -1, DDP_VOX_E_ALIGN = -2, DDP_VOX_E_LAUNCH = -3, DDP_VOX_E_NULL = -4' in header
    assert C.sizeof(M.Cfg) == 14 * 4 and [f[0] for f in M.Cfg._fields_] == ['batch', 'pmax', 'max_voxels', 'max_points', 'feats', 'grid', 'lo', 'vs']
    assert M.Cfg.grid.offset == 20 and M.Cfg.lo.offset == 32 and M.Cfg.vs.offset == 44


def test_stale_or_missing_library_raises(tmp_path, monkeypatch):
    with pytest.raises(M.DdpVoxError, match='not found'):
        M.load(str(tmp_path / 'libddp_vox.so'))
    monkeypatch.setattr(M._binding, 'libs', {})
    with monkeypatch.context() as m:
        m.setattr(build.LATER['vox'], 'built_hash', lambda: 'feedfeedfeedfeed')
        with pytest.raises(M.DdpVoxError, match='is stale'):
            M.load()
    monkeypatch.setattr(M._binding, 'abi_version', M.ABI_VERSION + 1)
    with pytest.raises(M.DdpVoxError, match='ABI mismatch: library 1 vs binding 2') as e:
        M.load()
    assert e.value.code is None and isinstance(e.value, RuntimeError) and not M._binding.libs


def test_the_documented_hash():
    assert M.hash_capacity(1) == 2 and M.hash_capacity(1024) == 2048 and M.hash_capacity(1025) == 4096 and M.hash_capacity(250000) == 524288
    assert M.home_slot(0, 100) == 0 and M.home_slot(1, 100) == 2654435761 >> 24 and M.home_slot(2 ** 31 - 1, 2 ** 20) < 2 ** 21
    ids = np.arange(4096, dtype=np.uint64)
    home = ((ids * np.uint64(M.HASH_MULT)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - 9)
    assert [M.home_slot(int(i), 256) for i in ids[:300]] == home[:300].tolist() and M.hash_capacity(256) == 512


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
FAKE = 0x10000    # a non-NULL, 256-byte aligned "device pointer": every call below is refused before anything is enqueued


def _cfg(**over):
    cfg = M.Cfg(2, 300, 50, 3, 5, (C.c_int32 * 3)(16, 24, 16), (C.c_float * 3)(0.0, -1.2, -0.6), (C.c_float * 3)(0.075, 0.1, 0.075))
    for k, v in over.items():
        if k in ('grid', 'lo', 'vs'):
            for j, x in enumerate(v):
                getattr(cfg, k)[j] = x
        else:
            setattr(cfg, k, v)
    return cfg


def _calls(cfg, points=(FAKE, FAKE), counts=(300, 0), stride=5, ws=FAKE, cells=FAKE, a=FAKE, b=FAKE, c=FAKE, only=None):
    lib = M.load()
    n = C.c_size_t(0)
    out = [C.c_void_p(0) for _ in range(5)]
    B = max(cfg.batch, 1)
    ptrs = (C.c_void_p * B)(*(list(points) + [FAKE] * B)[:B]) if points is not None else None
    cnts = (C.c_int32 * B)(*(list(counts) + [0] * B)[:B]) if counts is not None else None
    calls = dict(workspace=lambda: lib.ddp_vox_workspace(C.byref(cfg), C.byref(n)),
                 cells=lambda: lib.ddp_vox_cells(C.byref(cfg), ptrs, cnts, stride, ws, None),
                 assign=lambda: lib.ddp_vox_assign(C.byref(cfg), ws, None),
                 assign_from_cells=lambda: lib.ddp_vox_assign_from_cells(C.byref(cfg), cells, ws, None),
                 tables=lambda: lib.ddp_vox_tables(C.byref(cfg), ws, *[C.byref(p) for p in out]),
                 gather=lambda: lib.ddp_vox_gather(C.byref(cfg), ptrs, cnts, stride, ws, a, b, c, None),
                 pack=lambda: lib.ddp_vox_pack(C.byref(cfg), ptrs, cnts, stride, 1, ws, a, b, c, None),
                 pack_raw=lambda: lib.ddp_vox_pack(C.byref(cfg), ptrs, cnts, stride, 0, ws, a, b, c, None))
    return calls if only is None else calls[only]


def _refused(rc, code, words):
    msg = M.load().ddp_vox_last_error().decode()
    assert rc == code and words in msg, (rc, msg, words)


def test_refusals_happen_before_any_launch():
    """no GPU is present where this runs: a call that got as far as a launch would fail with DDP_VOX_E_LAUNCH, not with these"""
    inf, nan = float('inf'), float('nan')
    bad = [(dict(batch=0), 'batch'), (dict(batch=-2), 'batch'), (dict(pmax=0), 'pmax'), (dict(pmax=-2 ** 31), 'pmax'), (dict(max_voxels=0), 'max_voxels'),
           (dict(max_voxels=-1), 'DynamicScatter'), (dict(max_points=-1), 'DynamicScatter'), (dict(max_points=0), 'max_points'), (dict(feats=0), 'feats'),
           (dict(grid=(0, 24, 16)), 'grid[0]'), (dict(grid=(16, -1, 16)), 'grid[1]'), (dict(grid=(16, 24, 0)), 'grid[2]'),
           (dict(feats=17), 'feats = 17 exceeds 16'), (dict(max_points=257), 'max_points = 257 exceeds 256'),
           (dict(grid=(1 << 11, 1 << 10, 1 << 10)), 'grid volume'), (dict(grid=(46341, 46341, 1)), 'grid volume'), (dict(grid=(1 << 16, 1 << 16, 1 << 16)), 'grid volume'),
           (dict(batch=1 << 11, pmax=1 << 20), 'B*pmax'), (dict(batch=1 << 10, max_voxels=1 << 13, max_points=256), 'B*max_voxels*max_points'),
           (dict(batch=1 << 16, max_voxels=1 << 16, max_points=1), 'B*max_voxels*max_points'),
           (dict(batch=1, pmax=(1 << 29) + 1), 'B*H'), (dict(batch=4, pmax=1 << 28), 'B*H'),
           (dict(vs=(0.0, 0.1, 0.1)), 'vs[0]'), (dict(vs=(0.1, -0.1, 0.1)), 'vs[1]'), (dict(vs=(0.1, 0.1, inf)), 'vs[2]'), (dict(vs=(nan, 0.1, 0.1)), 'vs[0]'),
           (dict(lo=(nan, 0.0, 0.0)), 'lo[0]'), (dict(lo=(0.0, inf, 0.0)), 'lo[1]'), (dict(lo=(0.0, 0.0, -inf)), 'lo[2]')]
    for over, words in bad:
        for name, call in _calls(_cfg(**over)).items():
            _refused(call(), M.E_BADCFG, words)
    # just below the limits: accepted, and the recipe's size
    n = C.c_size_t(0)
    lib = M.load()
    assert lib.ddp_vox_workspace(C.byref(_cfg(batch=1, pmax=1 << 29, max_voxels=(1 << 23) - 1, max_points=256, feats=16, grid=(1 << 11, 1 << 10, (1 << 10) - 1))), C.byref(n)) == 0
    cfg = _cfg()
    for name in ('cells', 'gather', 'pack', 'pack_raw'):
        _refused(_calls(cfg, stride=4, only=name)(), M.E_BADCFG, 'stride = 4')
        _refused(_calls(_cfg(feats=2), stride=5, only=name)(), M.E_BADCFG, 'x, y, z')
        _refused(_calls(cfg, counts=(300, -1), only=name)(), M.E_BADCFG, 'count[1] = -1')
        _refused(_calls(cfg, counts=(301, 0), only=name)(), M.E_BADCFG, 'exceeds pmax')
        _refused(_calls(cfg, points=None, only=name)(), M.E_NULL, 'h_points is NULL')
        _refused(_calls(cfg, counts=None, only=name)(), M.E_NULL, 'h_counts is NULL')
        _refused(_calls(cfg, points=(None, None), only=name)(), M.E_NULL, 'h_points[b] is NULL')
        _refused(_calls(cfg, points=(FAKE + 2, FAKE), only=name)(), M.E_ALIGN, 'h_points[b] must be')
        # a sample without a point needs no pointer: the NULL of the second sample (count 0) is not what refuses this call
        _refused(_calls(cfg, points=(FAKE, None), ws=None, only=name)(), M.E_NULL, 'd_workspace is NULL')
    for name in ('cells', 'assign', 'assign_from_cells', 'tables', 'gather', 'pack'):
        _refused(_calls(cfg, ws=None, only=name)(), M.E_NULL, 'd_workspace is NULL')
        _refused(_calls(cfg, ws=FAKE + 128, only=name)(), M.E_ALIGN, 'd_workspace must be 256-byte')
    _refused(_calls(cfg, cells=None, only='assign_from_cells')(), M.E_NULL, 'd_cells is NULL')
    _refused(_calls(cfg, cells=FAKE + 2, only='assign_from_cells')(), M.E_ALIGN, 'd_cells must be')
    for name, outs in (('gather', ('d_voxels', 'd_coors', 'd_num_points')), ('pack', ('d_feats', 'd_coords', 'd_sizes'))):
        for key, what in zip('abc', outs):
            _refused(_calls(cfg, only=name, **{key: None})(), M.E_NULL, what + ' is NULL')
            _refused(_calls(cfg, only=name, **{key: FAKE + 1})(), M.E_ALIGN, what + ' must be 4-byte')
    _refused(lib.ddp_vox_workspace(None, C.byref(n)), M.E_NULL, 'cfg is NULL')
    _refused(lib.ddp_vox_workspace(C.byref(cfg), None), M.E_NULL, 'bytes is NULL')
    ptr = [C.byref(C.c_void_p(0)) for _ in range(5)]
    for i, what in enumerate(('d_cells', 'd_point_voxel', 'd_voxel_points', 'd_voxel_cells', 'd_counts')):
        _refused(lib.ddp_vox_tables(C.byref(cfg), FAKE, *[None if j == i else p for j, p in enumerate(ptr)]), M.E_NULL, what + ' is NULL')
    # the binding turns a refused configuration into ValueError, anything else into DdpVoxError
    with pytest.raises(ValueError, match='grid volume'):
        L.HardVoxelizer([0.001, 0.001, 0.001], [0, 0, 0, 2, 2, 2], 10, 100)
    with pytest.raises(ValueError, match='max_points = 300 exceeds 256'):
        L.HardVoxelizer([0.1, 0.1, 0.1], [0, 0, 0, 2, 2, 2], 300, 100)
    with pytest.raises(M.DdpVoxError, match='is NULL') as e:
        M.check(_calls(cfg, ws=None, only='assign')(), lib)
    assert e.value.code == M.E_NULL


def test_workspace_formula_knows_no_grid_volume_and_table_places():
    lib = M.load()
    r = lambda n: (n + 255) // 256 * 256
    for g, B, pmax, V, T in ((VC.G16, 1, 1, 5, 3), (VC.G32, 3, 1300, 350, 10), (VC.G_FLAT, 2, 1025, 7, 256), (VC.G_RECIPE, 1, 250000, 120000, 10),
                             (VC.G_RECIPE, 4, 250000, 120000, 10)):
        hv = L.HardVoxelizer(g['voxel_size'], g['range'], T, V)
        assert hv.grid == g['grid'] and hv.workspace_bytes(B, pmax, 5) == VC.workspace_bytes(B, pmax, V, T) == hv.workspace_bytes(B, pmax, 16)
        small = L.HardVoxelizer(VC.G16['voxel_size'], VC.G16['range'], T, V)
        assert small.workspace_bytes(B, pmax, 5) == hv.workspace_bytes(B, pmax, 5)                 # another grid, the same bytes
        ptrs = [C.c_void_p(0) for _ in range(5)]
        assert lib.ddp_vox_tables(C.byref(hv.cfg(B, pmax, 5)), FAKE, *[C.byref(p) for p in ptrs]) == 0
        P = B * pmax
        assert [p.value - FAKE for p in ptrs] == [0, r(4 * P), 2 * r(4 * P), 2 * r(4 * P) + r(4 * B * V * T), 2 * r(4 * P) + r(4 * B * V * T) + r(4 * B * V)]
    # the recipe's size: below 15 MB per sample, where a dense table over 1024 x 1024 x 40 cells alone would take 168 MB
    assert VC.workspace_bytes(1, 250000, 120000, 10) == 14573568 < 1024 * 1024 * 40 * 4 // 10


# ---- kernel resources ----------------------------------------------------------------------------------------------------------------
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
KERNELS = ['k_vox_cells', 'k_vox_take_cells', 'k_vox_clear', 'k_vox_insert', 'k_vox_tile_sums', 'k_vox_scan_sums', 'k_vox_number', 'k_vox_round0',
           'k_vox_round', 'k_vox_rows', 'k_vox_meta', 'k_vox_mean', 'k_vox_offsets']


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not available')
def test_no_kernel_touches_scratch(tmp_path):
    out = tmp_path / 'vox.s'
    src = os.path.join(build.LATER['vox'].csrc, 'ddp_vox.hip')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-x', 'hip', src,
                    '--cuda-device-only', '-S', '-o', str(out)], check=True, capture_output=True, timeout=600)
    figures = {}
    for m in re.finditer(r'\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel', out.read_text(), re.S):
        body = m.group(2)
        short = re.search(r'k_vox_[a-z_0-9]+?(?=E[a-zA-Z])', m.group(1)).group(0)
        figures[short] = tuple(int(re.search(rf'\.amdhsa_{key} (\d+)', body).group(1))
                               for key in ('private_segment_fixed_size', 'next_free_vgpr', 'group_segment_fixed_size'))
    print('kernel: (scratch B, VGPRs, static LDS B)', figures)
    assert sorted(figures) == sorted(KERNELS)
    for name, (scratch, vgpr, lds) in figures.items():
        assert scratch == 0, f'{name}: {scratch} B of scratch'
        assert vgpr <= 32, f'{name}: {vgpr} registers'
    assert {k: v[2] for k, v in figures.items() if v[2]} == {'k_vox_tile_sums': 16, 'k_vox_number': 16, 'k_vox_scan_sums': 1024}


# ---- plugin surface ------------------------------------------------------------------------------------------------------------------
def test_plugin_surface_is_the_reference_class():
    """the constructor arguments, members and ``__repr__`` of bev/mmdet3d/ops/voxel/voxelize.py ``Voxelization``"""
    import ddp_amd
    assert ddp_amd.Voxelization is Voxelization and 'Voxelization' in ddp_amd.__all__ and 'use_device_voxelization' in ddp_amd.__all__
    sig = inspect.signature(Voxelization.__init__).parameters
    assert list(sig)[1:] == ['voxel_size', 'point_cloud_range', 'max_num_points', 'max_voxels', 'deterministic']
    assert sig['max_voxels'].default == 20000 and sig['deterministic'].default is True
    vs, rng = [0.1, 0.1, 0.2], [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
    m = Voxelization(vs, rng, 10, [90000, 120000])
    assert m.voxel_size is vs and m.point_cloud_range is rng and m.max_num_points == 10 and m.max_voxels == (90000, 120000)
    m = Voxelization(vs, rng, 10, (90000, 120000), deterministic=False)
    assert m.max_voxels == (90000, 120000) and m.deterministic is False and isinstance(m, torch.nn.Module) and not list(m.state_dict())
    assert m.grid_size.dtype == torch.int64 and m.grid_size.tolist() == [1024, 1024, 40] and [int(v) for v in m.pcd_shape] == [1024, 1024, 1]
    assert repr(m) == ('Voxelization(voxel_size=[0.1, 0.1, 0.2], point_cloud_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], max_num_points=10, '
                       'max_voxels=(90000, 120000), deterministic=False)')
    assert Voxelization(vs, rng, 10).max_voxels == (20000, 20000)
    assert m.training and m.engine().max_voxels == 90000 and m.eval().engine().max_voxels == 120000 and m.engine() is m.engine()
    assert m.engine().max_num_points == 10 and m.engine().grid == [1024, 1024, 40]
    for kw in (dict(max_num_points=-1), dict(max_num_points=10, max_voxels=-1), dict(max_num_points=10, max_voxels=(-1, 100))):
        with pytest.raises(NotImplementedError, match='DynamicScatter'):
            Voxelization(vs, rng, **kw)
    with pytest.raises(NotImplementedError, match='DynamicScatter'):
        L.HardVoxelizer(vs, rng, 10, -1)


def test_cpu_tensors_fp16_and_backward_raise_and_points_stay():
    c = VC.case('dups')
    hv = L.HardVoxelizer(c['voxel_size'], c['range'], c['T'], c['max_voxels'])
    p = torch.from_numpy(c['points'][0])
    before = p.clone()
    for call in (lambda: hv.cells(p), lambda: hv.cells([p]), lambda: hv.voxelize(p), lambda: hv.voxelize_batch([p, p]),
                 lambda: hv.assign_from_cells(torch.zeros(1, 4, dtype=torch.int32)), lambda: Voxelization(c['voxel_size'], c['range'], 3, 50).eval()(p)):
        with pytest.raises(ValueError, match='no CPU path'):
            call()
    with pytest.raises(RuntimeError, match='call cells'):
        hv.assign()
    with pytest.raises(RuntimeError, match='call cells'):
        hv.tables()
    with pytest.raises(RuntimeError, match='call assign'):
        hv.gather()
    with pytest.raises(ValueError, match='non-empty list'):
        hv.cells([])
    with pytest.raises(ValueError, match='takes a list'):
        hv.voxelize([p])
    with pytest.raises(ValueError, match='must be a list'):
        hv.voxelize_batch(p)
    assert torch.equal(p, before)
    # fp16 and a tensor that asks for a gradient are refused by message, wherever they live
    with pytest.raises(NotImplementedError, match='fp16 points are not built'):
        hv.cells(p.half())
    with pytest.raises(NotImplementedError, match='no backward'):
        hv.voxelize_batch([p.clone().requires_grad_()])


class _Model:
    pass


def _stub(max_num_points=10, max_voxels=(90000, 120000), reduce=True, lidar=True):
    """a BEVFusion-shaped object without its constructor: ``encoders['lidar']['voxelize']`` and ``voxelize_reduce``"""
    model = object.__new__(_Model)
    old = object.__new__(_Model)
    old.voxel_size, old.point_cloud_range, old.max_num_points, old.max_voxels = [0.1, 0.1, 0.2], [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], max_num_points, max_voxels
    old.deterministic, old.training = False, False
    model.encoders = {'lidar': {'voxelize': old, 'backbone': 'kept'}} if lidar else {'camera': {}}
    model.voxelize_reduce = reduce
    return model, old


def test_use_device_voxelization_on_stub_models():
    model, old = _stub()
    assert registry.use_device_voxelization(model) is old
    new = model.encoders['lidar']['voxelize']
    assert isinstance(new, Voxelization) and model.encoders['lidar']['backbone'] == 'kept'
    assert (new.voxel_size, new.point_cloud_range, new.max_num_points, new.max_voxels, new.deterministic) == (old.voxel_size, old.point_cloud_range, 10, (90000, 120000), False)
    assert not new.training and new.engine().max_voxels == 120000
    assert inspect.ismethod(model.voxelize) and model.voxelize.__self__ is model
    with pytest.raises(ValueError, match='no CPU path'):                   # the bound method reaches the device engine
        model.voxelize([torch.zeros(3, 5)])
    # reduce: the model's own unless given
    for given, own, want in ((None, True, True), (None, False, False), (False, True, False), (True, False, True)):
        model, old = _stub(reduce=own)
        registry.use_device_voxelization(model, reduce=given)
        assert model.voxelize.__func__.__closure__ is not None
        assert [c.cell_contents for c in model.voxelize.__func__.__closure__ if isinstance(c.cell_contents, bool)] == [want]
    with pytest.raises(ValueError, match='no lidar encoder'):
        registry.use_device_voxelization(_stub(lidar=False)[0])
    with pytest.raises(ValueError, match='no lidar encoder'):
        registry.use_device_voxelization(object.__new__(_Model))
    for t in (-1, 0):
        model, old = _stub(max_num_points=t)
        with pytest.raises(NotImplementedError, match='only hard voxelisation'):
            registry.use_device_voxelization(model)
        assert model.encoders['lidar']['voxelize'] is old and not hasattr(model, 'voxelize')      # refused: nothing was replaced
    with pytest.raises(NotImplementedError, match='DynamicScatter'):
        registry.use_device_voxelization(_stub(max_voxels=(-1, -1))[0])
