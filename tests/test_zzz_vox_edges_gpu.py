"""The device-side hard voxelisation on an MI355X on the cases of tests/vox_edge_cases.py: the voxel cap across scan tiles and inside a
thread's run, more scan tiles than the one-block scan has threads, hash probing that wraps past the last slot, cell ids above 2^24 and
2^30, per-sample tables of a batch, T = 1 and T = 256, empty batches, and a ``HardVoxelizer`` that owns its workspace and re-plans.
Checked as tests/test_zz_vox_gpu.py checks (its ``Rig``, ``_check`` and ``_parts`` are used as they are): every workspace and output
buffer exactly sized, guarded and filled with ``support.PATTERN``; every integer output and ``voxels`` bit for bit against the
sequential restatement; the means inside ``vox_cases.mean_f64``'s bound and equal to the left-to-right fp32 sum.  No new tolerance.
THREE tests of named parts, collected behind tests/test_zz_vox_gpu.py: the GPU suite's earlier ids keep their places.  Reads only
tests/golden/, tests/vox_cases.py and tests/vox_edge_cases.py; what makes each case worth running is asserted in tests/test_vox_edges_host.py."""
import os

import numpy as np
import pytest
import torch

import parity_report
import vox_cases as VC
import vox_edge_cases as E
from ddp_amd import vox as L
from support import PATTERN, Guarded, assert_guards, dev  # noqa: F401
from test_zz_vox_gpu import Rig, _check, _parts

pytestmark = pytest.mark.gpu
PAT = np.int32(PATTERN)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vox')


# ---- the integer half: a caller's table through ``assign_from_cells`` -------------------------------------------------------------------
def _run_table(tc, V, dev, runs=1):
    """one voxelizer in an exactly sized, guarded, PATTERN-filled workspace; every table against ``assign_ref``, sample by sample;
    ``runs`` > 1: the workspace refilled before each, identical bytes required"""
    B, pmax, T = tc['B'], tc['pmax'], tc['T']
    what = f'{tc["name"]} max_voxels={V}'
    hv = L.HardVoxelizer(tc['voxel_size'], tc['range'], T, V)
    assert hv.grid == tc['grid']
    need = hv.workspace_bytes(B, pmax)
    assert need == VC.workspace_bytes(B, pmax, V, T), what
    ws = Guarded(need, dev)
    hv.use_workspace(ws.ws.view(torch.uint8))
    src = torch.from_numpy(tc['table']).to(dev)
    cells, refs = E.taken(tc), E.table_ref(tc, V)
    first = None
    for run in range(runs):
        ws.ws.view(torch.int32).fill_(PATTERN)
        hv.assign_from_cells(src)
        torch.cuda.synchronize()
        assert_guards(ws, what)
        gc, gp, gt, gv, gm = (t.cpu().numpy().copy() for t in hv.tables())
        assert gc.shape == gp.shape == (B, pmax) and gt.shape == (B, V, T) and gv.shape == (B, V) and gm.shape == (B,)
        assert gm.tolist() == [len(r[1]) for r in refs], f'{what}: counts {gm.tolist()}, expected {[len(r[1]) for r in refs]}'
        for b, (pvox, table, vcells) in enumerate(refs):
            m = len(table)
            assert np.array_equal(gc[b], cells[b]), f'{what} sample {b}: cells'
            bad = np.flatnonzero(gp[b] != pvox)
            assert not len(bad), f'{what} sample {b}: point_voxel differs at {len(bad)} rows, first {bad[:5].tolist()}: {gp[b][bad[:5]].tolist()} for {pvox[bad[:5]].tolist()}'
            assert np.array_equal(gt[b, :m], table) and (gt[b, m:] == -1).all(), f'{what} sample {b}: voxel_points'
            assert np.array_equal(gv[b, :m], vcells), f'{what} sample {b}: voxel_cells'
        state = b''.join([gc.tobytes(), gp.tobytes(), gt.tobytes(), gm.tobytes()] + [gv[b, :gm[b]].tobytes() for b in range(B)])
        first = first or state
        assert state == first, f'{what}: run {run} differs from run 0'
    assert torch.equal(src.cpu(), torch.from_numpy(tc['table'])), f'{what}: the caller\'s table was written'
    with pytest.raises(RuntimeError, match='made without points'):
        hv.gather()
    return gp, gt, gv, gm


def _every_cap(name, dev, runs=1):
    tc = E.case(name)
    return {V: _run_table(tc, V, dev, runs) for V in tc['caps']}


def _part_cap_tiles_the_cap_on_every_side_of_a_tile_border(dev):
    """kept cells still gain points after the cap was hit, dropped cells' points have no voxel, every table exact - for each of the
    eleven caps of the case"""
    got = _every_cap('cap_tiles', dev)
    total = E.CAP_TILES_HEAD + E.CAP_TILES_NEW
    assert [int(g[3][0]) for g in got.values()] == [1, 1023, 1024, 1025, 1026, 1027, 2047, 2048, 2049, total, total]


def _part_wrap_probing_past_the_last_slot(dev):
    _every_cap('wrap', dev, runs=3)
    _every_cap('wrap_small2', dev, runs=3)
    _every_cap('wrap_small3', dev, runs=3)


def _part_batch_tables_are_per_sample(dev):
    tc = E.case('batch_tables')
    for V, (gp, gt, gv, gm) in _every_cap('batch_tables', dev).items():
        voxel = [int(gp[b, at]) for b, at in enumerate((3, 41, 17))]       # one id in all three samples: a voxel of its own in each
        assert all(v >= 0 and gv[b, v] == tc['table'][0, 3] for b, v in enumerate(voxel)) or V == 10, (V, voxel)
    for V, (gp, gt, gv, gm) in _every_cap('batch_hollow', dev).items():
        assert gm[1] == 0 and (gp[1] == -1).all() and (gt[1] == -1).all(), V


def _part_big_ids_from_a_callers_table(dev):
    got = _every_cap('big_ids', dev, runs=2)
    assert sorted(got[20][2][0, :8].tolist()) == sorted(E.BIG_IDS)


def _part_scan257_two_tile_sums_per_thread(dev):
    gp, gt, gv, gm = _every_cap('scan257', dev)[106000]
    assert gm[0] < 106000 == gm[1] and gp[0, -1] == gm[0] - 1 and gp[1, -1] == -1


def _part_scan600_three_tile_sums_per_thread(dev):
    gp, gt, gv, gm = _every_cap('scan600', dev)[250000]
    assert gm.tolist() == [250000] and gp[0, -1] == -1


# ---- the point half and the host layer ------------------------------------------------------------------------------------------------------
def _run_points(name, dev, pmax=None):
    ref = E.reference(name)
    rig = Rig(ref['c'], dev, pmax=pmax)
    got = rig.run()
    try:
        ratio = _check(ref, got)
    except AssertionError as e:
        raise AssertionError(f'case {name}: {e}') from e
    return ref, got, ratio


def _part_cap_batch_samples_on_both_sides_of_the_cap(dev):
    ref, got, ratio = _run_points('cap_batch', dev, pmax=E.CAP_BATCH_PMAX)
    assert got['counts'].tolist() == [900, 1100, 1100] and got['cells'].shape == (3, E.CAP_BATCH_PMAX)
    for key in ('coords', 'coords_raw'):                                   # the pack offsets follow the counts
        assert np.flatnonzero(np.diff(got[key][:3100, 0])).tolist() == [899, 1999] and got[key][3099, 0] == 2
    fix = VC.load_fixture('cap_batch', GOLDEN)                             # the reference's own arrays
    for b in range(3):
        m = int(got['counts'][b])
        assert got['voxels'][b, :m].tobytes() == fix[f'voxels{b}'].tobytes() and np.array_equal(got['coors'][b, :m], fix[f'coors{b}'])
        assert np.array_equal(got['num'][b, :m], fix[f'num{b}'])
    rows = len(fix['sizes'])
    assert rows == got['counts'].sum() and np.array_equal(got['coords'][:rows], fix['coords']) and np.array_equal(got['sizes'][:rows], fix['sizes'])
    assert got['raw'][:rows].tobytes() == fix['feats_raw'].tobytes()
    want, bound = ref['mean64']
    assert (np.abs(fix['feats'].astype(np.float64) - want) <= bound).all()
    parity_report.record(f'vox cap_batch: exact on cells, voxels, coors, num_points, coords, sizes; largest |device mean - f64| / ((n + 1) 2^-24 '
                         f'sum|x| / n) = {ratio:.4f}; source: reference fixture + restatement')


def _part_big_ids_through_points(dev):
    for name, last in (('big_points', (2047, 1023, 1022)), ('recipe_corners', (1023, 1023, 39))):
        ref, got, ratio = _run_points(name, dev)
        m = int(got['counts'][0])
        assert m == 9 and got['cells'].max() == E.volume(ref['c']) - 1 and last in set(map(tuple, got['coors'][0, :m].tolist()))
        assert last in set(map(tuple, got['coords'][:m, 1:].tolist()))
    assert got['cells'].max() == 41943039


def _part_T1_no_round_kernels(dev):
    ref, got, ratio = _run_points('T1', dev)
    m = int(got['counts'][0])
    assert m == 40 and (got['sizes'][:m] == 1).all() and (got['num'][0, :m] == 1).all()
    rows = ref['c']['points'][0][got['table'][0, :m, 0]]
    assert got['feats'][:m].tobytes() == rows.tobytes() and ratio == 0.0   # the mean of one row is that row, bit for bit


def _part_T256_the_point_limit(dev):
    ref, got, ratio = _run_points('T256', dev)
    m = int(got['counts'][0])
    assert m == len(E.T256_ROWS) and sorted(got['num'][0, :m].tolist()) == sorted(min(n, 256) for n in E.T256_ROWS)
    assert got['voxels'].shape == (1, 8, 256, 16) and got['voxels'][0, :m].tobytes() == ref['per'][0][0].tobytes()
    print(f'T256: largest |device mean - f64| / bound at n = 256: {ratio:.4f}')
    parity_report.record(f'vox T256: exact on the (M, 256, 16) rows; largest |device mean - f64| / ((n + 1) 2^-24 sum|x| / n) = {ratio:.4f} '
                         f'(n up to 256; 0.49 at n <= 10); source: restatement')


def _part_empty_batches(dev):
    ref, got, ratio = _run_points('all_empty', dev)
    assert got['counts'].tolist() == [0, 0, 0]
    for key in ('voxels', 'coors', 'num', 'feats', 'coords', 'sizes', 'raw', 'coords_raw', 'sizes_raw'):      # nothing was written
        assert (got[key].view(np.int32) == PAT).all(), key
    ref, got, ratio = _run_points('ends_empty', dev)
    m = int(got['counts'][1])
    assert got['counts'].tolist() == [0, m, 0] and m == len(ref['sizes']) > 40
    for key in ('coords', 'coords_raw'):
        assert (got[key][:m, 0] == 1).all() and np.array_equal(got[key][:m, 1:], ref['per'][1][1]) and (got[key][m:] == PAT).all(), key
    assert got['raw'][:m].tobytes() == ref['per'][1][0].tobytes()         # the rows start at 0


def _call(hv, kind, rows, dev):
    """-> the bytes-comparable result of one call, cloned: the returned tensors are views of the voxelizer's buffers"""
    if kind == 'one':
        out = hv.voxelize(torch.from_numpy(rows).to(dev))
    else:
        out = hv.voxelize_batch([torch.from_numpy(r).to(dev) for r in rows], reduce=True)
    return [t.clone().cpu().numpy() for t in out] + [t.clone().cpu().numpy() for t in hv.tables()]


def _part_replan_of_an_owned_workspace(dev):
    """large -> small -> B = 3 -> large -> B = 3 in another order on ONE voxelizer that owns its workspace: each result equals a fresh
    voxelizer's byte for byte, and the restatement"""
    c = VC.case('tiles4097')
    make = lambda: L.HardVoxelizer(c['voxel_size'], c['range'], c['T'], c['max_voxels'])
    hv = make()
    for step, (kind, rows) in enumerate(E.replan_calls()):
        got, fresh = _call(hv, kind, rows, dev), _call(make(), kind, rows, dev)
        assert len(got) == len(fresh) == 8
        counts = got[7].tolist()
        for i, (a, b) in enumerate(zip(got, fresh)):
            if i == 6:                                                     # voxel cells beyond M_b are not written
                a, b = [np.concatenate([t[s, :n] for s, n in enumerate(counts)]) for t in (a, b)]
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), f'call {step} ({kind}): output {i} differs from a fresh voxelizer\'s'
        if kind == 'one':
            voxels, coors, num = VC.hard_voxelize_ref(rows, c)
            assert got[0].tobytes() == voxels.tobytes() and np.array_equal(got[1], coors) and np.array_equal(got[2], num), f'call {step}'
        else:
            feats, coords, sizes = VC.batch_ref(dict(c, points=list(rows), counts=[len(r) for r in rows], B=len(rows)))
            assert np.array_equal(got[0], feats) and np.array_equal(got[1], coords) and np.array_equal(got[2], sizes), f'call {step}'
            assert len(sizes) > 3000 and sorted(set(coords[:, 0].tolist())) == [0, 1, 2]


# ---- the three tests ---------------------------------------------------------------------------------------------------------------------
def test_integer_half_cap_across_tiles_wrap_batch_tables_big_ids(dev):
    """``assign_from_cells``: the voxel cap on every side of a scan-tile border and inside a thread's run, probing that wraps past slot
    H - 1, per-sample tables of a batch, ids above 2^24 and 2^30"""
    _parts([_part_cap_tiles_the_cap_on_every_side_of_a_tile_border, _part_wrap_probing_past_the_last_slot, _part_batch_tables_are_per_sample,
            _part_big_ids_from_a_callers_table], dev)


def test_scan_of_more_tile_sums_than_threads(dev):
    """257 and 600 scan tiles per sample: two and three tile sums per thread of the one-block scan, the cap crossed beyond tile 200 / 500"""
    _parts([_part_scan257_two_tile_sums_per_thread, _part_scan600_three_tile_sums_per_thread], dev)


def test_point_half_limits_empty_batches_and_replan(dev):
    """a batch on both sides of the cap, corner cells of a 2^31-cell grid and of the recipe's, T = 1, T = 256, empty batches, and a
    voxelizer that owns its workspace across re-plans"""
    _parts([_part_cap_batch_samples_on_both_sides_of_the_cap, _part_big_ids_through_points, _part_T1_no_round_kernels, _part_T256_the_point_limit,
            _part_empty_batches, _part_replan_of_an_owned_workspace], dev)
