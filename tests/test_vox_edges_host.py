"""CPU side of tests/vox_edge_cases.py (tests/test_zzz_vox_edges_gpu.py runs the cases on an MI355X): every case holds the witness its
name promises - where the voxel cap falls among the scan tiles and inside a thread's run of 4 points, more tiles than the one-block
scan has threads, keys that can only sit in slots reached by wrapping, ids above 2^24 and 2^30; every case DISCRIMINATES - a
restatement with one defect built in (``vox_edge_cases.assign_scan``) differs from ``assign_ref`` / ``cells_ref`` on it, which stands in
for mutating the kernel; the scan-form restatement without a defect equals ``assign_ref``; the workspace formula and the hash capacity
of every new shape.  No GPU compute is invoked."""
import json
import os

import numpy as np
import pytest

import vox_cases as VC
import vox_edge_cases as E
from ddp_amd import _vox_lib as M
from ddp_amd import vox as L

TILE = E.SCAN_TILE
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vox')


def founder_rows(cells):
    """the rows that found a cell, ascending: founder number v is at ``founder_rows(cells)[v]``"""
    uniq, first = np.unique(cells, return_index=True)
    return np.sort(first[uniq >= 0])


def place(row):
    """-> (tile, thread, position in the thread's run)"""
    return row // TILE, row % TILE // E.PER_THREAD, row % E.PER_THREAD


def same(a, b):
    return len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


# ---- the module's own constants and models ---------------------------------------------------------------------------------------------
def test_constants_hash_and_capacity_are_the_bindings():
    assert (E.HASH_MULT, E.SCAN_TILE) == (M.HASH_MULT, M.SCAN_TILE) and E.THREADS * E.PER_THREAD == M.SCAN_TILE and E.PER_THREAD == 4
    want = {5123: 16384, 2500: 8192, 256 * 1024 + 1: 1 << 20, 599 * 1024 + 1: 1 << 21, 400: 1024, 2: 4, 3: 8, 70: 256, 40: 128, 1: 2}
    for pmax, H in want.items():
        assert M.hash_capacity(pmax) == E.capacity(pmax) == H, pmax
    ids = np.asarray([0, 1, 2 ** 16, 2 ** 24 + 1, 2 ** 30 + 1, 2 ** 31 - 1, E.volume(E.G_BIG) - 1, E.volume(VC.G_RECIPE) - 1])
    for pmax in want:
        assert E.homes(ids, pmax).tolist() == [M.home_slot(int(i), pmax) for i in ids], pmax
    assert not set(E.TABLE_NAMES + E.POINT_NAMES) & set(VC.NAMES) and len(VC.NAMES) == 27 and VC.NAMES[0] == 'one' and VC.NAMES[-1] == 'batch'
    assert [E.case(n)['seed'] for n in E.TABLE_NAMES] == list(range(2000, 2000 + len(E.TABLE_NAMES)))


@pytest.mark.parametrize('name', E.TABLE_NAMES)
def test_scan_form_without_a_defect_equals_the_sequential_loop(name):
    tc = E.case(name)
    for V in tc['caps']:
        for b, cells in enumerate(E.taken(tc)):
            got = E.assign_scan(cells, tc['T'], V)
            assert same(got, E.table_ref(tc, V)[b]) and got[3] == len(E.table_ref(tc, V)[b][1]), (V, b)


# ---- witnesses ---------------------------------------------------------------------------------------------------------------------------
def test_cap_tiles_puts_the_cap_on_every_side_of_a_tile_border():
    tc = E.case('cap_tiles')
    cells = E.taken(tc)[0]
    total = E.CAP_TILES_HEAD + E.CAP_TILES_NEW
    rows = founder_rows(cells)
    assert tc['pmax'] == 5 * TILE + 3 and tc['T'] == 3 and tc['B'] == 1 and tc['grid'] == [1024, 1024, 40]
    assert len(rows) == total and rows[:E.CAP_TILES_HEAD].tolist() == list(range(E.CAP_TILES_HEAD))   # founder number = row index
    assert tc['caps'] == [1, 1023, 1024, 1025, 1026, 1027, 2047, 2048, 2049, total, total + 1]
    assert (cells == -1).sum() >= 100 and cells.max() > 2 ** 24
    # the cap-th founder (the last one kept) and the first one dropped: (tile, thread, position in the thread's run of 4)
    last_kept = {1: (0, 0, 0), 1023: (0, 255, 2), 1024: (0, 255, 3), 1025: (1, 0, 0), 1026: (1, 0, 1), 1027: (1, 0, 2), 2047: (1, 255, 2),
                 2048: (1, 255, 3), 2049: (2, 0, 0)}
    first_dropped = {1: (0, 0, 1), 1023: (0, 255, 3), 1024: (1, 0, 0), 1025: (1, 0, 1), 1026: (1, 0, 2), 1027: (1, 0, 3), 2047: (1, 255, 3),
                     2048: (2, 0, 0), 2049: (2, 0, 1)}
    nt = (tc['pmax'] + TILE - 1) // TILE
    starts = np.asarray([(rows < t * TILE).sum() for t in range(nt)])
    tile_of = rows // TILE
    for V in tc['caps']:
        pvox, table, vcells = E.table_ref(tc, V)[0]
        assert len(table) == min(V, total)
        if V >= total:
            assert not ((pvox == -1) & (cells >= 0)).any()                  # the cap is never hit, even where it equals the founders
            continue
        assert place(int(rows[V - 1])) == last_kept[V] and place(int(rows[V])) == first_dropped[V], V
        assert (starts >= V).any() and (starts[1:] == V).any() == (V in (1024, 2048)), V      # a tile that starts at or above the cap
        r = int(rows[V])
        later = np.arange(len(cells)) > r
        # points of a kept cell that come after the cap was hit are still added, and reach the voxel's rows while it has room
        assert (later & (pvox >= 0)).sum() >= (20 if V > 1 else 4) and (table[:, 1:] > r).sum() >= (10 if V > 1 else 2), V
        # a founder of a LATER TILE is dropped and its cell comes back: those points have no voxel either
        dropped = rows[V:]
        back = [f for f in dropped.tolist() if f // TILE > r // TILE and (cells[f + 1:] == cells[f]).any()]
        assert len(back) >= 50 and all((pvox[cells == cells[f]] == -1).all() for f in back), V
        # repeats of ids founded around the two borders, kept or dropped by this cap
        for f in list(range(1020, 1031)) + list(range(2040, 2052)):
            assert (cells == cells[f]).sum() == 5 and (pvox[cells == cells[f]] == (f if f < V else -1)).all(), (V, f)
    assert len(set(tile_of.tolist())) == nt - 1 or len(set(tile_of.tolist())) == nt


@pytest.mark.parametrize('name, pmax, B, cap, tile_from', [('scan257', 256 * 1024 + 1, 2, 106000, 200), ('scan600', 599 * 1024 + 1, 1, 250000, 500)])
def test_scan_cases_have_more_tiles_than_the_scan_has_threads(name, pmax, B, cap, tile_from):
    tc = E.case(name)
    nt = (pmax + TILE - 1) // TILE
    assert (tc['pmax'], tc['B'], tc['caps'], tc['T']) == (pmax, B, [cap], 2) and nt > E.THREADS and pmax % TILE == 1
    per = (nt + E.THREADS - 1) // E.THREADS
    # the one-block scan of the tile sums gives a thread ``per`` entries: 2 of 257 (threads >= 129 have none), 3 of 600 (>= 200 idle)
    assert (nt, per, -(-nt // per)) == ((257, 2, 129) if name == 'scan257' else (600, 3, 200))
    crossing = {}
    for b, cells in enumerate(E.taken(tc)):
        rows = founder_rows(cells)
        pvox, table, vcells = E.table_ref(tc, cap)[b]
        assert 0.04 < (cells == -1).mean() < 0.06 and cells.max() > 2 ** 24
        assert (rows // TILE >= E.THREADS).sum() >= 1 and rows[-1] == pmax - 1        # the last row, alone in its tile, founds a cell
        if len(rows) <= cap:
            assert pvox[-1] == len(rows) - 1 == len(table) - 1                          # its number: the sum of all earlier tiles
            assert not ((pvox == -1) & (cells >= 0)).any()
            continue
        r = int(rows[cap])
        crossing[b] = r // TILE
        assert r // TILE >= tile_from and len(table) == cap and pvox[-1] == -1
        later = np.arange(pmax) > r
        dropped = set(cells[rows[cap:]].tolist())
        repeats = np.asarray([c in dropped for c in cells[r + 1:].tolist()]) & ~np.isin(np.arange(r + 1, pmax), rows)
        assert len(rows) - cap >= 1000 and repeats.sum() >= 500 and (later & (pvox >= 0)).sum() >= 1000
    assert crossing == ({1: 222} if name == 'scan257' else {0: 532}), crossing


def test_scan257_takes_two_entries_per_thread():
    """257 tiles over 256 threads: ``per`` = 2, the clamped ``lo`` / ``hi`` leave threads 129 .. 255 without an entry"""
    nt = 257
    per = (nt + E.THREADS - 1) // E.THREADS
    lo = [min(t * per, nt) for t in range(E.THREADS)]
    hi = [min(l + per, nt) for l in lo]
    assert per == 2 and hi[128] - lo[128] == 1 and all(h == l == nt for l, h in zip(lo[129:], hi[129:]))


def test_wrap_keys_must_sit_in_slots_reached_by_wrapping():
    tc = E.case('wrap')
    H = E.capacity(E.WRAP_PMAX)
    cells = E.taken(tc)[0]
    ids = np.asarray(sorted(set(cells[cells >= 0].tolist())))
    home = E.homes(ids, E.WRAP_PMAX)
    assert (tc['pmax'], H, tc['T'], tc['caps'], tc['grid']) == (400, 1024, 3, [120], [128, 128, 128])
    assert [(home == s).sum() for s in (H - 3, H - 2, H - 1)] == [32, 32, 32] and len(ids) == 104
    assert sorted(home[home < H - 3].tolist()) == [0, 0, 1, 2, 3, 3, 4, 5]
    raw = tc['table'][0].astype(np.int64)
    assert all((raw == v).sum() == 1 for v in (E.volume(E.G128), E.INT_MAX, E.INT_MIN)) and (cells >= 0).sum() == 96 * 3 + 8
    assert all((cells == i).sum() == 3 for i in ids[home >= H - 3])
    # whatever the arrival order: three slots hold three keys, the other 93 of the last homes sit in slots 0 .. reached by wrapping
    rng = np.random.default_rng(5)
    for order in [None, np.arange(400)[::-1]] + [rng.permutation(400) for _ in range(3)]:
        slot = E.slots_ref(cells, E.WRAP_PMAX, order)
        wrapped = [i for i, h in zip(ids.tolist(), home.tolist()) if h >= H - 3 and slot[i] < H - 3]
        assert len(slot) == 104 and len(wrapped) >= 93 and max(slot[i] for i in wrapped) >= 93 - 1
        assert sorted(slot.values()) == list(range(101)) + [H - 3, H - 2, H - 1]            # which slots are taken does not depend on the order
        moved = [i for i, h in zip(ids.tolist(), home.tolist()) if h < H - 3 and slot[i] != h]
        assert len(moved) >= 2                                             # ids with homes 0 .. 5 are displaced by the wrapped run
    pvox, table, vcells = E.table_ref(tc, 120)[0]
    assert len(table) == 104 and (table >= 0).sum() == 96 * 3 + 8
    for pmax in (2, 3):
        tc = E.case(f'wrap_small{pmax}')
        H = E.capacity(pmax)
        assert H == 2 ** pmax and tc['B'] == 2 and tc['pmax'] == pmax and (E.homes(tc['table'].reshape(-1), pmax) == H - 1).all()
        assert len(set(tc['table'][0].tolist())) == pmax and len(set(tc['table'][1].tolist())) == pmax - 1
        assert sorted(E.slots_ref(tc['table'][0], pmax).values()) == sorted([0, H - 1] + [1] * (pmax - 2))


def test_batch_tables_share_ids_across_samples():
    tc, hollow = E.case('batch_tables'), E.case('batch_hollow')
    first = [int(np.flatnonzero(row == tc['table'][0, 3])[0]) for row in tc['table']]
    assert tc['B'] == hollow['B'] == 3 and first == [3, 41, 17] and (hollow['table'][1] == -1).all()
    assert np.array_equal(hollow['table'][[0, 2]], tc['table'][[0, 2]])
    for V in tc['caps']:
        refs = E.table_ref(tc, V)
        voxel = [int(r[0][at]) for r, at in zip(refs, first)]
        assert len(set(voxel)) == 3 or V == 10, voxel                      # one id, three voxel numbers: the tables are per sample
        assert [len(r[1]) for r in E.table_ref(hollow, V)][1] == 0
    counts = [len(r[1]) for r in E.table_ref(tc, 10)]
    assert counts == [10, 10, 10] and all(((r[0] == -1) & (row >= 0)).any() for r, row in zip(E.table_ref(tc, 10), tc['table']))
    assert all(25 < len(r[1]) < 45 for r in E.table_ref(tc, 45)) and len({len(r[1]) for r in E.table_ref(tc, 45)}) > 1


def test_big_ids_exceed_what_a_float_holds():
    tc = E.case('big_ids')
    vol = E.volume(E.G_BIG)
    assert vol == 2145386496 < 2 ** 31 and tc['volume'] == vol and tc['grid'] == [2048, 1024, 1023]
    assert E.BIG_IDS == (0, 2 ** 24, 2 ** 24 + 1, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, vol - 2, vol - 1)
    raw, cells = tc['table'][0], E.taken(tc)[0]
    assert set(raw.tolist()) == set(E.BIG_IDS) | {vol, -1} and (raw == vol).sum() == 3 and set(cells.tolist()) == set(E.BIG_IDS) | {-1}
    assert sorted((cells == i).sum() for i in E.BIG_IDS) == [1, 1, 2, 2, 3, 3, 4, 4]
    assert sum(i > 2 ** 24 for i in E.BIG_IDS) == 6 and sum(i > 2 ** 30 for i in E.BIG_IDS) == 3
    assert sum(int(np.float32(i)) != i for i in E.BIG_IDS) == 5            # ids a float32 does not hold
    assert len(E.table_ref(tc, 5)[0][1]) == 5 and len(E.table_ref(tc, 20)[0][1]) == 8
    # through points: every corner cell and one in the middle, ids by int64 arithmetic
    for name, g, mid in (('big_points', E.G_BIG, (1023, 511, 1022)), ('recipe_corners', VC.G_RECIPE, (511, 1023, 20))):
        c = E.case(name)
        gx, gy, gz = g['grid']
        want = sorted([(x * gy + y) * gz + z for x in (0, gx - 1) for y in (0, gy - 1) for z in (0, gz - 1)] + [(mid[0] * gy + mid[1]) * gz + mid[2]])
        cells = VC.cells_ref(c['points'][0], c)
        assert sorted(set(cells.tolist())) == want and c['counts'] == [18] and (np.bincount(np.unique(cells, return_inverse=True)[1]) == 2).all()
        voxels, coors, num = VC.hard_voxelize_ref(c['points'][0], c)
        assert len(coors) == 9 and (num == 2).all() and sorted(map(tuple, coors.tolist()))[-1] == (gx - 1, gy - 1, gz - 1)
        assert want[-1] == E.volume(g) - 1 and (want[-1] == 41943039 or name == 'big_points')


# ---- the point half ------------------------------------------------------------------------------------------------------------------
def test_point_cases_keep_their_promises():
    c = E.case('cap_batch')
    per = [VC.hard_voxelize_ref(p, c) for p in c['points']]
    feats, coords, sizes = VC.batch_ref(c)
    assert (c['B'], c['T'], c['max_voxels'], c['grid']) == (3, 4, 1100, [32, 36, 32]) and max(c['counts']) <= E.CAP_BATCH_PMAX == 2500
    founders = [founder_rows(VC.cells_ref(p, c)) for p in c['points']]
    assert [len(f) for f in founders] == [900, 1100, 1700] and [len(v) for v, _, _ in per] == [900, 1100, 1100]
    assert founders[2][1100] // TILE == 1 and founders[1][-1] // TILE == 1                  # the last sample crosses the cap in tile 1
    assert np.flatnonzero(np.diff(coords[:, 0])).tolist() == [899, 1999] and len(coords) == 3100    # the pack offsets follow the counts
    pvox = VC.assign_ref(VC.cells_ref(c['points'][2], c), 4, 1100)[0]
    assert (pvox[founders[2][1100]:] >= 0).any() and (pvox == -1).sum() >= 600
    c = E.case('T1')
    pvox, table, vcells = VC.assign_ref(VC.cells_ref(c['points'][0], c), c['T'], c['max_voxels'])
    feats, coords, sizes = VC.batch_ref(c)
    assert c['counts'] == [300] and c['T'] == 1 and table.shape == (40, 1) and (sizes == 1).all()
    assert feats.tobytes() == c['points'][0][table[:, 0]].tobytes()                         # the mean of one row is that row
    c = E.case('T256')
    cells = VC.cells_ref(c['points'][0], c)
    pvox, table, vcells = VC.assign_ref(cells, c['T'], c['max_voxels'])
    assert (c['T'], c['F'], c['stride'], c['counts']) == (M.MAX_POINTS, M.MAX_FEATS, 19, [1100]) and sorted(np.bincount(pvox)) == sorted(E.T256_ROWS)
    assert sorted((table >= 0).sum(1)) == sorted(min(n, 256) for n in E.T256_ROWS) and (np.diff(np.flatnonzero(pvox == pvox[0])) > 1).any()
    c = E.case('all_empty')
    assert c['counts'] == [0, 0, 0] and len(VC.batch_ref(c)[2]) == 0
    c = E.case('ends_empty')
    feats, coords, sizes = VC.batch_ref(c)
    assert c['counts'] == [0, 60, 0] and len(sizes) > 40 and (coords[:, 0] == 1).all()
    calls = E.replan_calls()
    assert [k for k, _ in calls] == ['one', 'one', 'batch', 'one', 'batch'] and [len(calls[i][1]) for i in (0, 1, 3)] == [4097, 10, 4097]
    assert [len(p) for p in calls[2][1]] == [1500, 7, 2590] == [len(p) for p in calls[4][1]][::-1]


def test_cap_batch_fixture_equals_the_restatement_bit_for_bit():
    """the reference's own ``hard_voxelize_cpu`` and ``BEVFusion.voxelize`` on the batch that ends on both sides of the cap"""
    assert E.FIXTURES == ['cap_batch']
    c, fix = E.case('cap_batch'), VC.load_fixture('cap_batch', GOLDEN)
    assert json.loads(str(fix['config'])) == json.loads(VC.config_of(c)) and c['grid'][0] == c['grid'][2]
    assert os.path.getsize(os.path.join(GOLDEN, 'vox_cap_batch.npz')) <= os.path.getsize(os.path.join(GOLDEN, 'vox_batch.npz'))
    for b, p in enumerate(c['points']):
        voxels, coors, num = VC.hard_voxelize_ref(p, c)
        assert fix[f'points{b}'].tobytes() == p.tobytes() and fix[f'voxels{b}'].dtype == np.float32
        assert fix[f'voxels{b}'].shape == voxels.shape and fix[f'voxels{b}'].tobytes() == voxels.tobytes()
        assert fix[f'coors{b}'].dtype == fix[f'num{b}'].dtype == np.int32 and np.array_equal(fix[f'coors{b}'], coors) and np.array_equal(fix[f'num{b}'], num)
    feats, coords, sizes = VC.batch_ref(c, reduce=True)
    raw = VC.batch_ref(c, reduce=False)[0]
    assert np.array_equal(fix['coords'], coords) and np.array_equal(fix['sizes'], sizes) and fix['feats_raw'].tobytes() == raw.tobytes()
    want, bound = VC.mean_f64(raw, sizes)
    assert fix['feats'].shape == feats.shape and (np.abs(fix['feats'].astype(np.float64) - want) <= bound).all()


# ---- every case discriminates --------------------------------------------------------------------------------------------------------
SHOWS = {'sums_past_256': [('scan257', 106000, 0), ('scan257', 106000, 1), ('scan600', 250000, 0)],
         'cap_per_tile': [('cap_tiles', V, 0) for V in (1, 1023, 1024, 1025, 2047, 2048, 2049)] + [('scan257', 106000, 1), ('scan600', 250000, 0)],
         'cap_per_run': [('cap_tiles', V, 0) for V in (1, 1023, 1025, 1026, 1027, 2047, 2049)],
         'probe_stops': [('wrap', 120, 0), ('wrap_small2', 5, 0), ('wrap_small3', 5, 0), ('wrap_small3', 5, 1)],
         'id_through_float': [('big_ids', 5, 0), ('big_ids', 20, 0)],
         'dropped_to_last': [('cap_tiles', V, 0) for V in (1, 1023, 1024, 1027, 2048, 2049)] + [('scan257', 106000, 1), ('scan600', 250000, 0),
                                                                                                ('batch_tables', 10, 0), ('batch_tables', 10, 2), ('big_ids', 5, 0)]}


@pytest.mark.parametrize('defect', E.DEFECTS)
def test_a_restatement_with_the_defect_differs_on_the_case(defect):
    assert sorted(SHOWS) == sorted(E.DEFECTS)
    for name, V, b in SHOWS[defect]:
        tc = E.case(name)
        assert V in tc['caps']
        bad = E.assign_scan(E.taken(tc)[b], tc['T'], V, defect)
        assert not same(bad, E.table_ref(tc, V)[b]), (defect, name, V, b)


def test_the_run_defect_hides_where_the_cap_falls_on_a_run_border():
    """the cap test made once per run of 4 is right when the cap is a multiple of 4: why cap_tiles has 1023 and 1025 .. 1027 too"""
    tc = E.case('cap_tiles')
    for V in (1024, 2048):
        assert same(E.assign_scan(E.taken(tc)[0], tc['T'], V, 'cap_per_run'), E.table_ref(tc, V)[0])


def test_a_cell_id_formed_in_float_differs_on_the_corner_cells():
    for name in ('big_points', 'recipe_corners'):
        c = E.case(name)
        lo, vs, grid = np.asarray(c['range'][:3], np.float32), np.asarray(c['voxel_size'], np.float32), np.asarray(c['grid'], np.float32)
        q = np.floor((c['points'][0][:, :3] - lo) / vs).astype(np.float32)
        bad = ((q[:, 0] * grid[1] + q[:, 1]) * grid[2] + q[:, 2]).astype(np.float32).astype(np.int64)
        assert (bad != VC.cells_ref(c['points'][0], c)).any(), name


# ---- formulas ------------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_of_every_new_shape():
    shapes = [(tc, tc['B'], tc['pmax'], V, tc['T']) for tc in map(E.case, E.TABLE_NAMES) for V in tc['caps']]
    shapes += [(c, c['B'], max(c['counts'] + [1]), c['max_voxels'], c['T']) for c in map(E.case, E.POINT_NAMES)]
    shapes += [(E.case('cap_batch'), 3, E.CAP_BATCH_PMAX, 1100, 4)]
    for c, B, pmax, V, T in shapes:
        hv = L.HardVoxelizer(c['voxel_size'], c['range'], T, V)
        assert hv.grid == c['grid'] and hv.workspace_bytes(B, pmax, 3) == VC.workspace_bytes(B, pmax, V, T) == hv.workspace_bytes(B, pmax, 16), c['name']
    for name in ('scan257', 'scan600'):
        tc = E.case(name)
        assert 30e6 < VC.workspace_bytes(tc['B'], tc['pmax'], tc['caps'][0], tc['T']) < 36e6
